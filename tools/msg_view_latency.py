#!/usr/bin/env python3
"""What a decoded-view call costs on an MI355X: nwc_sanitize_messages_view against
nwc_sanitize_messages_ex on the same binary, and the untouched plain path against the parent
commit's library.

    python tools/msg_view_latency.py [--out profiles/msg_view/msg_view_latency.json]
    python tools/msg_view_latency.py --ab abtest/libnwc_parent.so [--out profiles/msg_view/plain_ab.json]

Method.  The messages are k valid headers of 67 parents from a committee of 100, k = 1, 16, 99, as
tools/batch_vote_latency.py builds them.  Route "ex": nwc_sanitize_messages_ex without per-message
arrays and without a signer.  Route "view": nwc_sanitize_messages_view on the same arguments with
views, a body of nwc_msg_view_body_bound bytes and body_used.  Wall clock (perf_counter) around each
whole call, which ends with every output in host memory.  The routes alternate in rounds after a
warm-up round of each; p50 / p99 over all timed calls of a route, spread = max - min of the
per-round p50s.  Before anything is timed the view call's codes, digests and kinds are compared
with the _ex call's and every view with the wire (round, author, id, parents' offset).
Large batch: the 20,000 messages (6,667 headers of 67 parents, 13,333 votes; 18.3 MB, one staged
chunk) of profiles/batch_vote, one _view and one _ex call alternating; k_message_views' own time is
taken as p50(view) - p50(ex), which also holds the records' copy back.
--ab: the untouched path, as tools/batch_vote_latency.py --ab: p50 of plain nwc_sanitize_messages
over 16 headers in child processes that load the parent commit's library and this build's
(NWC_LIB_PATH) in the order A B B A.
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import batch_vote_latency as bv  # noqa: E402

KS = (1, 16, 99)


class ViewBatch(bv.Batch):
    def __init__(self, lib, msgs):
        import numpy as np
        super().__init__(msgs)
        self.cap = int(lib.nwc_msg_view_body_bound(int(self.offs[-1]), self.m))
        self.views = np.zeros((self.m, 160), np.uint8)
        self.body = np.zeros(self.cap, np.uint8)
        self.used = ctypes.c_uint64(0)


def routes(args):
    import torch
    from narwhal_amd import _lib
    from narwhal_amd import build as nb
    assert torch.cuda.is_available(), "msg_view_latency.py measures on a GPU"
    lib = _lib.load()
    orc, pks, hdrs, votes = bv.world(100, max(KS), 67, 198)
    bv.install(lib, pks)
    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "), "rounds": args.rounds, "k": {}}

    def ex(b):
        rc = lib.nwc_sanitize_messages_ex(_lib.buf(b.data), _lib.buf(b.offs), b.m, None, 0, None, None, None, _lib.buf(b.codes),
                                          _lib.buf(b.dig), _lib.buf(b.kinds), None, None)
        assert rc == 0

    def view(b):
        rc = lib.nwc_sanitize_messages_view(_lib.buf(b.data), _lib.buf(b.offs), b.m, None, 0, None, None, None, _lib.buf(b.codes),
                                            _lib.buf(b.dig), _lib.buf(b.kinds), None, None, _lib.buf(b.views), _lib.buf(b.body),
                                            b.cap, ctypes.byref(b.used))
        assert rc == 0

    def check(b, expect):
        """the two routes' outputs agree, and every view names its message's fields in the wire"""
        ex(b)
        want = (b.codes.copy(), b.dig.copy(), b.kinds.copy())
        b.codes[:], b.dig[:], b.kinds[:] = -1, 0, 9
        view(b)
        assert (b.codes == want[0]).all() and (b.dig == want[1]).all() and (b.kinds == want[2]).all() and not b.codes.any()
        for i in range(b.m):
            v = _lib.MsgView.from_buffer_copy(b.views[i].tobytes())
            wire, (kind, hid, rnd, author) = b.msgs[i], expect(i)
            assert (v.decoded, v.kind, v.code, v.round) == (1, kind, 0, rnd) and bytes(v.id) == hid and bytes(v.author) == author
            assert v.author_index == pks.index(author)
            if kind == 1:
                assert v.sig_off + 64 == len(wire)
            if kind == 0:
                assert (v.flags, v.n_payload, v.n_parents, v.n_votes) == (0, 0, 67, 0)
                assert v.parents_off + 32 * 67 + 32 == v.sig_off and wire[v.parents_off + 32 * 67:v.sig_off] == hid

    names = {"ex": ex, "view": view}
    for k in KS:
        b = ViewBatch(lib, [h[0] for h in hdrs[:k]])
        check(b, lambda i: (0, hdrs[i][1], hdrs[i][2], hdrs[i][3]))
        per_round = max(1, args.calls // args.rounds)
        times, p50s = {n: [] for n in names}, {n: [] for n in names}
        for rnd in range(args.rounds + 1):
            for name, route in names.items():
                ts = []
                for i in range(per_round if rnd else max(50, per_round // 10)):
                    t0 = time.perf_counter()
                    route(b)
                    ts.append(time.perf_counter() - t0)
                if rnd:
                    times[name] += ts
                    p50s[name].append(bv.pct(ts, 0.5))
        row = {n: dict(bv.summary(times[n]), round_p50_spread_us=(max(p50s[n]) - min(p50s[n])) * 1e6) for n in names}
        row["view_minus_ex_p50_us"] = row["view"]["p50_us"] - row["ex"]["p50_us"]
        row["view_slower_by_more_than_ex_spread"] = row["view_minus_ex_p50_us"] > row["ex"]["round_p50_spread_us"]
        row["body_used"] = int(b.used.value)
        row["d2h_view_bytes_per_message"] = (160 * b.m + b.used.value) / b.m
        row["wire_bytes_per_message"] = int(b.offs[-1]) / b.m
        res["k"][str(k)] = row
        print(k, json.dumps(row), flush=True)

    # ---- the large batch of profiles/batch_vote
    M = 20000
    msgs = [hdrs[(i // 3) % len(hdrs)][0] if i % 3 == 0 else votes[i % len(votes)] for i in range(M)]
    b = ViewBatch(lib, msgs)

    def expect(i):
        if i % 3 == 0:
            h = hdrs[(i // 3) % len(hdrs)]
            return 0, h[1], h[2], h[3]
        w = msgs[i]
        assert struct.unpack_from("<Q", w, 36)[0] == 9
        return 1, w[4:36], 9, pks[(i % len(votes)) % 100]
    check(b, expect)
    t = {"view": [], "ex": []}
    for rnd in range(args.large_rounds + 2):
        for name in ("view", "ex"):
            t0 = time.perf_counter()
            names[name](b)
            if rnd >= 2:
                t[name].append(time.perf_counter() - t0)
    v, e = bv.pct(t["view"], 0.5), bv.pct(t["ex"], 0.5)
    res["large_batch"] = {"messages": M, "bytes": int(b.offs[-1]), "view_p50_ms": v * 1e3, "ex_p50_ms": e * 1e3,
                          "view_p99_ms": bv.pct(t["view"], 0.99) * 1e3, "ex_p99_ms": bv.pct(t["ex"], 0.99) * 1e3,
                          "view_spread_ms": (max(t["view"]) - min(t["view"])) * 1e3, "ex_spread_ms": (max(t["ex"]) - min(t["ex"])) * 1e3,
                          "k_message_views_and_copy_ms": (v - e) * 1e3, "share_of_view_call": (v - e) / v,
                          "body_used": int(b.used.value), "d2h_view_bytes_per_message": (160 * M + b.used.value) / M,
                          "wire_bytes_per_message": int(b.offs[-1]) / M,
                          "view_ms": [x * 1e3 for x in t["view"]], "ex_ms": [x * 1e3 for x in t["ex"]]}
    print(json.dumps({k: x for k, x in res["large_batch"].items() if not k.endswith("_ms") or "p50" in k or "copy" in k}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--large-rounds", type=int, default=10)
    ap.add_argument("--ab", default=None, help="the parent commit's library, relative to the repository root")
    ap.add_argument("--ab-rounds", type=int, default=4)
    args = ap.parse_args()
    if args.ab:
        res = bv.ab(args)   # (the child processes are batch_vote_latency.py --plain-child)
        out = args.out or os.path.join(ROOT, "profiles", "msg_view", "plain_ab.json")
    else:
        res = routes(args)
        out = args.out or os.path.join(ROOT, "profiles", "msg_view", "msg_view_latency.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("rounds", "method", "large_batch")}))


if __name__ == "__main__":
    main()
