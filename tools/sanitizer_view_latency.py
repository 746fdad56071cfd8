#!/usr/bin/env python3
"""Latency of getting the device's decode of a sanitized message on an MI355X from the sanitizer
handle: the route a node has without nwc_sanitizer_sanitize_view against the view from the group
flight.

    python tools/sanitizer_view_latency.py [--out profiles/sanitizer_view/view_latency.json]
    python tools/sanitizer_view_latency.py --ab abtest/libnwc_parent.so [--out profiles/sanitizer_view/plain_ab.json]

Method.  Two messages from a committee of 100: a valid header of 67 parents, and a valid config-3
certificate (that header with 67 votes).  The sanitizer is created with (0, 0), so a lone caller
launches at once and a burst shares what arrived together.  Route (a): nwc_sanitizer_sanitize, then
nwc_sanitize_messages_view on the one message -- what a node at the parent commit has if it wants
the device's decode.  Route (b): nwc_sanitizer_sanitize_view.  Route (c): plain
nwc_sanitizer_sanitize, to show what the view costs on top.  Wall clock (perf_counter) around each
whole route, which ends with every output in host memory.  The routes alternate in rounds (after a
warm-up round of each); p50 / p99 over all timed calls of a route, spread = max - min of the
per-round p50s.  One thread: --calls calls per route.  16 threads: bursts of 16 distinct messages
released by a barrier, one per thread, --calls calls per route in all; a call's time runs from its
thread's release to its return, a burst's from the release to the last return.  Before anything is
timed the record and body_used of route (b) are compared with route (a)'s (the tests compare the body).  A difference
between (a) and (b) smaller than route (a)'s own spread is reported as no difference.
The Byzantine case: flights of 8 headers released together, with and without a header of 600
unsorted payload entries among them (all asking for views); the burst's time, recorded, not bounded.
--ab: the untouched path.  Lone-header p50 of plain nwc_sanitizer_sanitize in child processes that
load the parent commit's library and this build's (NWC_LIB_PATH) in the order A B B A, --ab-rounds
times each; rounds are compared within the state a process landed in (profiles/vote/NOTES.md), and
the allowed margin is the spread of the parent's rounds of that state against each other.
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vote_latency import ab, install, pct, summary  # noqa: E402  (ab: its child is vote_latency.py's plain lone-header loop)


def world(n_committee, n_msgs, parents, votes):
    """n_msgs (header wire, certificate wire) pairs and a header of 600 unsorted payload entries."""
    import numpy as np
    import messages_ref as mr
    from tests.oracle_lib import load_oracle
    orc = load_oracle()
    rng = np.random.default_rng(2028)
    r32 = lambda: bytes(rng.integers(0, 256, 32, dtype=np.uint8))   # noqa: E731
    seeds = [r32() for _ in range(n_committee)]
    pks = [orc.public_key(s) for s in seeds]
    hdrs, certs = [], []
    for k in range(n_msgs):
        ps = [r32() for _ in range(parents)]
        hid = mr.header_id(pks[k], 5 + k, [], ps)
        hdr = mr.enc_header(pks[k], 5 + k, [], ps, hid, orc.sign(seeds[k], hid))
        cd = mr.digest72(hid, 5 + k, pks[k])
        hdrs.append(mr.msg_header(hdr))
        certs.append(mr.msg_certificate(hdr, [(pks[v], orc.sign(seeds[v], cd)) for v in range(votes)]))
    unsorted = [(r32(), j) for j in range(600)]
    byz = mr.msg_header(mr.enc_header(pks[0], 9, unsorted, [r32()], r32(), bytes(64), wire_order=True))
    return orc, pks, hdrs, certs, byz


def routes(args):
    import ctypes
    import numpy as np
    import torch
    from narwhal_amd import _lib
    from narwhal_amd import build as nb
    assert torch.cuda.is_available(), "sanitizer_view_latency.py measures on a GPU"
    lib = _lib.load()
    T = 16
    orc, pks, hdrs, certs, byz = world(100, T, 67, 67)
    install(lib, pks)
    san = lib.nwc_sanitizer_create(0, 0)
    assert san, lib.nwc_last_error()

    class Ctx:   # one thread's buffers
        def __init__(self, cap):
            self.dig, self.kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
            self.rec, self.body, self.cap = np.zeros(160, np.uint8), np.zeros(cap, np.uint8), cap
            self.used, self.code, self.offs = ctypes.c_uint64(0), np.zeros(1, np.int32), np.zeros(2, np.uint64)
            self.args = (_lib.buf(self.rec), _lib.buf(self.body), cap, ctypes.byref(self.used))

    def route_a(c, wire):
        assert lib.nwc_sanitizer_sanitize(san, _lib.buf(wire), len(wire), 0, None, c.dig, c.kind) >= 0
        c.offs[1] = len(wire)
        assert lib.nwc_sanitize_messages_view(_lib.buf(wire), _lib.buf(c.offs), 1, None, 0, None, None, None, _lib.buf(c.code),
                                              None, None, None, None, *c.args) == 0

    def route_b(c, wire):
        assert lib.nwc_sanitizer_sanitize_view(san, None, _lib.buf(wire), len(wire), 0, None, c.dig, c.kind, None, None,
                                               *c.args) >= 0

    def route_c(c, wire):
        assert lib.nwc_sanitizer_sanitize(san, _lib.buf(wire), len(wire), 0, None, c.dig, c.kind) == 0

    names = {"a": route_a, "b": route_b, "c": route_c}
    cap = max(len(b) for b in hdrs + certs + [byz]) + 64
    c0 = Ctx(cap)
    for wire in hdrs + certs + [byz]:
        route_a(c0, wire)
        want = (c0.rec.tobytes(), int(c0.used.value))
        c0.rec[:] = 0
        route_b(c0, wire)
        assert (c0.rec.tobytes(), int(c0.used.value)) == want

    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "), "rounds": args.rounds,
           "bytes": {"header": len(hdrs[0]), "certificate": len(certs[0]), "byzantine_header": len(byz)}}

    def diffs(d):
        d["b_minus_a_p50_us"] = d["b"]["p50_us"] - d["a"]["p50_us"]
        d["b_minus_c_p50_us"] = d["b"]["p50_us"] - d["c"]["p50_us"]
        d["b_differs_from_a"] = abs(d["b_minus_a_p50_us"]) > d["a"]["round_p50_spread_us"]
        return d

    for what, msgs in (("header", hdrs), ("certificate", certs)):
        # ---- one thread
        per_round = max(1, args.calls // args.rounds)
        times = {n: [] for n in names}
        p50s = {n: [] for n in names}
        for rnd in range(args.rounds + 1):
            for name, route in names.items():
                ts = []
                for _ in range(per_round if rnd else max(100, per_round // 10)):
                    t0 = time.perf_counter()
                    route(c0, msgs[0])
                    ts.append(time.perf_counter() - t0)
                if rnd:
                    times[name] += ts
                    p50s[name].append(pct(ts, 0.5))
        one = diffs({n: dict(summary(times[n]), round_p50_spread_us=(max(p50s[n]) - min(p50s[n])) * 1e6) for n in names})
        res[what + "_threads_1"] = one
        print(what, 1, json.dumps(one), flush=True)

        # ---- 16 threads, bursts of 16 distinct messages
        many = bursts_of(T, names, lambda name, k: msgs[k], lambda: Ctx(cap), max(1, args.calls // T // args.rounds), args.rounds)
        res[what + "_threads_16"] = diffs(many)
        print(what, 16, json.dumps(many), flush=True)

    # ---- the Byzantine case: 8 viewers per flight, one of them the 600-unsorted-entry header or not
    flights = max(10, args.calls // 80)
    byzr = bursts_of(8, {"honest": route_b, "byzantine": route_b},
                     lambda name, k: byz if (name == "byzantine" and k == 0) else hdrs[k], lambda: Ctx(cap), flights, args.rounds)
    byzr["byzantine_minus_honest_burst_p50_us"] = byzr["byzantine"]["burst_p50_us"] - byzr["honest"]["burst_p50_us"]
    res["byzantine_flight_of_8"] = byzr
    print("byzantine", json.dumps(byzr), flush=True)

    st = (ctypes.c_uint64 * 8)()
    vs = (ctypes.c_uint64(0), ctypes.c_uint64(0))
    assert lib.nwc_sanitizer_stats(san, st) == 0
    assert lib.nwc_sanitizer_view_stats(san, ctypes.byref(vs[0]), ctypes.byref(vs[1])) == 0
    res["sanitizer"] = {"groups": int(st[0]), "messages": int(st[1]), "redone_messages": int(st[4]),
                        "max_messages_in_group": int(st[6]), "views_in_flight": int(vs[0].value), "views_alone": int(vs[1].value)}
    assert lib.nwc_sanitizer_destroy(san) == 0
    return res


def bursts_of(T, names, pick, make_ctx, bursts, rounds):
    """T threads (thread k sends pick(route name, k)), `bursts` bursts per route and round released by a barrier; per route the calls'
    p50 / p99, the spread of the round p50s and the bursts' p50 / p99."""
    plan = [(rnd, name) for rnd in range(rounds + 1) for name in names]
    start, done = threading.Barrier(T + 1), threading.Barrier(T + 1)
    call_t = {key: [] for key in plan}
    lock = threading.Lock()

    def count(rnd):
        return bursts if rnd else max(10, bursts // 10)

    def worker(k):
        c = make_ctx()
        for rnd, name in plan:
            wire = pick(name, k)
            mine = []
            for _ in range(count(rnd)):
                start.wait()
                t0 = time.perf_counter()
                names[name](c, wire)
                mine.append(time.perf_counter() - t0)
                done.wait()
            with lock:
                call_t[(rnd, name)] += mine
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(T)]
    for t in threads:
        t.start()
    burst_t = {key: [] for key in plan}
    for rnd, name in plan:
        for _ in range(count(rnd)):
            start.wait()
            t0 = time.perf_counter()
            done.wait()
            burst_t[(rnd, name)].append(time.perf_counter() - t0)
    for t in threads:
        t.join()
    out = {}
    for name in names:
        calls = [x for rnd in range(1, rounds + 1) for x in call_t[(rnd, name)]]
        bs = [x for rnd in range(1, rounds + 1) for x in burst_t[(rnd, name)]]
        rp = [pct(call_t[(rnd, name)], 0.5) for rnd in range(1, rounds + 1)]
        out[name] = dict(summary(calls), round_p50_spread_us=(max(rp) - min(rp)) * 1e6, burst_p50_us=pct(bs, 0.5) * 1e6,
                         burst_p99_us=pct(bs, 0.99) * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab", default=None, help="the parent commit's library, relative to the repository root")
    ap.add_argument("--ab-rounds", type=int, default=6)
    args = ap.parse_args()
    if args.ab:
        res = ab(args)
        out = args.out or os.path.join(ROOT, "profiles", "sanitizer_view", "plain_ab.json")
    else:
        res = routes(args)
        out = args.out or os.path.join(ROOT, "profiles", "sanitizer_view", "view_latency.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("rounds", "method")}))


if __name__ == "__main__":
    main()
