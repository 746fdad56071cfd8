#!/usr/bin/env python3
"""Latency of voting for the headers of a batch on an MI355X: the two-call route a node has with
nwc_sanitize_messages against one nwc_sanitize_messages_ex call that carries the signer.

    python tools/batch_vote_latency.py [--out profiles/batch_vote/batch_vote_latency.json]
    python tools/batch_vote_latency.py --ab abtest/libnwc_parent.so [--out profiles/batch_vote/plain_ab.json]

Method.  The messages are k valid headers of 67 parents from a committee of 100, k = 1, 16, 99.
Route (a): nwc_sanitize_messages with digests, then the host decodes (id, round, author) of every Ok
header from its wire bytes (the base64 author included), then nwc_signer_vote_many.  Route (b):
nwc_sanitize_messages_ex with the signer (no per-message arrays: the same state for every message,
as route (a) has).  Wall clock (perf_counter) around each whole route, which ends with the
signatures in host memory.  The routes alternate in rounds after a warm-up round of each; p50 / p99
over all timed calls of a route, spread = max - min of the per-round p50s.  Every signature of both
routes is compared with the C restatement of dalek before anything is timed, and the two routes'
with each other after every round.
Large batch: 20,000 messages, a third of them headers (the rest votes), one _ex call with and one
without the signer, alternating; k_vote_msgs' share = (p50 with - p50 without) / p50 with.
--ab: the untouched path.  p50 of plain nwc_sanitize_messages over 16 headers in child processes
that load the parent commit's library and this build's (NWC_LIB_PATH) in the order A B B A,
--ab-rounds times each; the allowed margin is the spread of the parent's own rounds.
"""
import argparse
import base64
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

KS = (1, 16, 99)


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def summary(ts):
    return {"p50_us": pct(ts, 0.5) * 1e6, "p99_us": pct(ts, 0.99) * 1e6, "calls": len(ts)}


def world(n_committee, n_headers, parents, n_votes=0):
    import numpy as np
    import messages_ref as mr
    from tests.oracle_lib import load_oracle
    orc = load_oracle()
    rng = np.random.default_rng(2028)
    r32 = lambda: bytes(rng.integers(0, 256, 32, dtype=np.uint8))   # noqa: E731
    seeds = [r32() for _ in range(n_committee)]
    pks = [orc.public_key(s) for s in seeds]
    hdrs = []
    for k in range(n_headers):
        ps = [r32() for _ in range(parents)]
        hid = mr.header_id(pks[k], 5 + k, [], ps)
        wire = mr.msg_header(mr.enc_header(pks[k], 5 + k, [], ps, hid, orc.sign(seeds[k], hid)))
        hdrs.append((wire, hid, 5 + k, pks[k]))
    votes = []
    for k in range(n_votes):
        hid, origin = r32(), pks[(k + 1) % n_committee]
        a = k % n_committee
        votes.append(mr.msg_vote(hid, 9, origin, pks[a], orc.sign(seeds[a], mr.digest72(hid, 9, origin))))
    return orc, pks, hdrs, votes


def install(lib, pks):
    import ctypes
    from narwhal_amd import _lib
    n = len(pks)
    _lib.check(lib.nwc_set_committee_config(_lib.buf(b"".join(pks)), (ctypes.c_uint64 * n)(*([1] * n)), n,
                                            (ctypes.c_uint32 * (n + 1))(*range(n + 1)), (ctypes.c_uint32 * n)(*([0] * n))))


class Batch:
    """One batch's wire bytes and output buffers."""

    def __init__(self, msgs):
        import numpy as np
        self.msgs = msgs
        self.m = len(msgs)
        self.offs = np.zeros(self.m + 1, np.uint64)
        self.offs[1:] = np.cumsum([len(b) for b in msgs])
        self.data = np.frombuffer(b"".join(msgs), np.uint8).copy()
        self.codes = np.zeros(self.m, np.int32)
        self.dig = np.zeros((self.m, 32), np.uint8)
        self.kinds = np.zeros(self.m, np.uint8)
        self.sigs = np.zeros((self.m, 64), np.uint8)
        self.voted = np.zeros(self.m, np.uint8)


def host_decode(wire):
    """(round, author) of a header's wire bytes, as a node decodes them again on the CPU."""
    (n,) = struct.unpack_from("<Q", wire, 4)
    author = base64.b64decode(wire[12:12 + n])[:32]
    (rnd,) = struct.unpack_from("<Q", wire, 12 + n)
    return rnd, author


def plain_child(args):
    """One process, one library: p50 of plain nwc_sanitize_messages over 16 headers."""
    from narwhal_amd import _lib
    lib = _lib.load()
    orc, pks, hdrs, _ = world(100, 16, 67)
    install(lib, pks)
    b = Batch([h[0] for h in hdrs])
    ts = []
    for i in range(args.calls + args.calls // 10):
        t0 = time.perf_counter()
        rc = lib.nwc_sanitize_messages(_lib.buf(b.data), _lib.buf(b.offs), b.m, 0, None, _lib.buf(b.codes), _lib.buf(b.dig),
                                       _lib.buf(b.kinds))
        ts.append(time.perf_counter() - t0)
        assert rc == 0 and not b.codes.any()
    assert all(bytes(b.dig[k]) == hdrs[k][1] for k in range(16))
    print(json.dumps(dict(summary(ts[args.calls // 10:]), build_id=lib.nwc_build_id().decode())))


def ab(args):
    libs = {"parent": os.path.join(ROOT, args.ab), "this": os.path.join(ROOT, "narwhal_amd", "libnwc.so")}
    rows = {"parent": [], "this": []}
    order = []
    for r in range(args.ab_rounds):
        order += ["parent", "this"] if r % 2 == 0 else ["this", "parent"]
    for name in order:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--calls", str(args.calls)],
                             env=dict(os.environ, NWC_LIB_PATH=libs[name]), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        row = json.loads(out.stdout.strip().splitlines()[-1])
        rows[name].append(row)
        print(name, json.dumps(row), flush=True)
    p = sorted(x["p50_us"] for x in rows["parent"])
    t = sorted(x["p50_us"] for x in rows["this"])
    res = {"what": "p50 of nwc_sanitize_messages over 16 headers of 67 parents, committee of 100", "order": order,
           "rounds": rows, "parent_p50s_us": p, "this_p50s_us": t, "parent_p50_us": pct(p, 0.5), "this_p50_us": pct(t, 0.5),
           "parent_spread_us": max(p) - min(p)}
    res["this_minus_parent_us"] = res["this_p50_us"] - res["parent_p50_us"]
    res["within_margin"] = res["this_minus_parent_us"] <= res["parent_spread_us"]
    return res


def routes(args):
    import numpy as np
    import torch
    from narwhal_amd import _lib
    from narwhal_amd import build as nb
    import messages_ref as mr
    assert torch.cuda.is_available(), "batch_vote_latency.py measures on a GPU"
    lib = _lib.load()
    orc, pks, hdrs, votes = world(100, max(KS), 67, 198)
    install(lib, pks)
    seed = bytes(range(1, 33))
    signer = lib.nwc_signer_create(_lib.buf(seed + orc.public_key(seed)))
    assert signer, lib.nwc_last_error()
    want = [orc.sign(seed, mr.digest72(hid, rnd, author)) for _, hid, rnd, author in hdrs]
    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "), "rounds": args.rounds, "k": {}}

    def route_a(b):
        rc = lib.nwc_sanitize_messages(_lib.buf(b.data), _lib.buf(b.offs), b.m, 0, None, _lib.buf(b.codes), _lib.buf(b.dig),
                                       _lib.buf(b.kinds))
        assert rc == 0
        ok = [i for i in range(b.m) if b.codes[i] == 0 and b.kinds[i] == 0]
        dec = [host_decode(b.msgs[i]) for i in ok]
        ids = np.ascontiguousarray(b.dig[ok])
        rounds = np.array([d[0] for d in dec], np.uint64)
        origins = np.frombuffer(b"".join(d[1] for d in dec), np.uint8)
        out = np.zeros((len(ok), 64), np.uint8)
        assert lib.nwc_signer_vote_many(signer, _lib.buf(ids), _lib.buf(rounds), _lib.buf(origins), len(ok), _lib.buf(out)) == 0
        b.sigs[:] = 0
        b.sigs[ok] = out

    def route_b(b):
        rc = lib.nwc_sanitize_messages_ex(_lib.buf(b.data), _lib.buf(b.offs), b.m, None, 0, None, None, signer, _lib.buf(b.codes),
                                          _lib.buf(b.dig), _lib.buf(b.kinds), _lib.buf(b.sigs), _lib.buf(b.voted))
        assert rc == 0

    names = {"a": route_a, "b": route_b}
    for k in KS:
        b = Batch([h[0] for h in hdrs[:k]])
        for route in names.values():
            route(b)
            assert all(bytes(b.sigs[i]) == want[i] for i in range(k)), (route.__name__, k)
        per_round = max(1, args.calls // args.rounds)
        times = {"a": [], "b": []}
        p50s = {"a": [], "b": []}
        for rnd in range(args.rounds + 1):
            for name, route in names.items():
                ts = []
                for i in range(per_round if rnd else max(50, per_round // 10)):
                    t0 = time.perf_counter()
                    route(b)
                    ts.append(time.perf_counter() - t0)
                assert all(bytes(b.sigs[i]) == want[i] for i in range(k)), (name, k)
                if rnd:
                    times[name] += ts
                    p50s[name].append(pct(ts, 0.5))
        row = {n: dict(summary(times[n]), round_p50_spread_us=(max(p50s[n]) - min(p50s[n])) * 1e6) for n in names}
        row["b_minus_a_p50_us"] = row["b"]["p50_us"] - row["a"]["p50_us"]
        row["b_faster_by_more_than_a_spread"] = -row["b_minus_a_p50_us"] > row["a"]["round_p50_spread_us"]
        res["k"][str(k)] = row
        print(k, json.dumps(row), flush=True)

    # ---- the vote launch's share of a large batch
    M = 20000
    msgs = [hdrs[(i // 3) % len(hdrs)][0] if i % 3 == 0 else votes[i % len(votes)] for i in range(M)]
    b = Batch(msgs)
    t = {"with": [], "without": []}

    def ex(with_signer):
        rc = lib.nwc_sanitize_messages_ex(_lib.buf(b.data), _lib.buf(b.offs), b.m, None, 0, None, None,
                                          signer if with_signer else None, _lib.buf(b.codes), _lib.buf(b.dig), _lib.buf(b.kinds),
                                          _lib.buf(b.sigs) if with_signer else None, _lib.buf(b.voted) if with_signer else None)
        assert rc == 0 and not b.codes.any()
    for rnd in range(args.large_rounds + 2):
        for name in ("with", "without"):
            t0 = time.perf_counter()
            ex(name == "with")
            if rnd >= 2:
                t[name].append(time.perf_counter() - t0)
    ex(True)
    hi = [i for i in range(M) if i % 3 == 0]
    assert b.voted[hi].all() and int(b.voted.sum()) == len(hi)
    assert all(bytes(b.sigs[i]) == want[(i // 3) % len(hdrs)] for i in hi)
    assert not b.sigs[b.voted == 0].any()
    w, wo = pct(t["with"], 0.5), pct(t["without"], 0.5)
    res["large_batch"] = {"messages": M, "headers": len(hi), "bytes": int(b.offs[-1]), "with_signer_p50_ms": w * 1e3,
                          "without_signer_p50_ms": wo * 1e3, "vote_launch_ms": (w - wo) * 1e3, "vote_share": (w - wo) / w,
                          "with_signer_ms": [x * 1e3 for x in t["with"]], "without_signer_ms": [x * 1e3 for x in t["without"]]}
    print(json.dumps({k: v for k, v in res["large_batch"].items() if not k.endswith("signer_ms")}), flush=True)
    assert lib.nwc_signer_destroy(signer) == 0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--large-rounds", type=int, default=10)
    ap.add_argument("--ab", default=None, help="the parent commit's library, relative to the repository root")
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--plain-child", action="store_true")
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    if args.ab:
        res = ab(args)
        out = args.out or os.path.join(ROOT, "profiles", "batch_vote", "plain_ab.json")
    else:
        res = routes(args)
        out = args.out or os.path.join(ROOT, "profiles", "batch_vote", "batch_vote_latency.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("rounds", "method", "large_batch")}))


if __name__ == "__main__":
    main()
