#!/usr/bin/env python3
"""One-message sanitize calls from many threads on an MI355X: nwc_sanitize_messages with m = 1 (one
call at a time per device) against a sanitizer (nwc_sanitizer: concurrent messages share one
pipeline launch), same binary.

    python tools/sanitizer_rate.py [--out profiles/sanitizer/sanitizer_rate.json]

Method.  One process, T = 1, 2, 4, 8, 16 Python threads (ctypes releases the GIL around a call;
never more than 16 threads).  A committee of 100 single-stake authorities (quorum 67), signed for by
the CPU oracle.  Every call carries one wire message; four legs: "certificate" = config-3 shape (2
parents, 67 votes, ~8 KB) from a pool of 64 distinct certificates cycled (verdicts are not cached,
so reuse is fair); "header" = a header of 67 parents; "vote"; "mix" = the three 1 : 1 : 1.  For
every leg and T, rounds alternate between route A = nwc_sanitize_messages(m = 1) and route B =
nwc_sanitizer_sanitize on one sanitizer created with (0, 0): --rounds timed rounds of --seconds
each after one warm-up round of both.  A round starts all threads at a barrier; each thread calls
back to back until the round's time is up and times every call with perf_counter.  Reported per leg,
T and route: calls/s over all timed rounds, the per-round calls/s and their spread (max - min), p50
/ p99 of the per-call latency over all timed calls, the spread of the per-round p50s, and for B the
mean messages per group (from nwc_sanitizer_stats).  Every answer is checked (all messages are
valid; one corrupted message per leg must come back InvalidSignature on both routes).  The
environment's NWC_SANITIZER_* switches (the group's bytes and messages) are recorded with the
result, so a sweep is one run per setting.  The Python loop costs a few
microseconds per call under the GIL, which bounds what 16 threads can show.
"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

STATS = ("groups", "messages", "bytes", "equations", "redone_messages", "bypassed_messages", "max_messages_in_group")


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sanitizer", "sanitizer_rate.json"))
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", default="1,2,4,8,16")
    ap.add_argument("--legs", default="certificate,header,vote,mix")
    ap.add_argument("--route", default="AB", help="AB = alternate both; B = the sanitizer alone (for a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import messages_ref as mr
    from narwhal_amd import _lib
    from narwhal_amd import build as nb
    from tests.oracle_lib import load_oracle
    assert torch.cuda.is_available(), "sanitizer_rate.py measures on a GPU"
    threads = [int(x) for x in args.threads.split(",")]
    assert max(threads) <= 16
    lib = _lib.load()
    orc = load_oracle()
    rng = np.random.default_rng(2027)
    N, POOL = 100, 64
    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "), "seconds_per_round": args.seconds,
           "rounds": args.rounds, "switches": {k: v for k, v in os.environ.items() if k.startswith("NWC_SANITIZER_")},
           "legs": {}}

    seeds = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(N)]
    pks = [orc.public_key(s) for s in seeds]
    kb = b"".join(pks)
    _lib.check(lib.nwc_set_committee_config(_lib.buf(kb), (ctypes.c_uint64 * N)(*([1] * N)), N,
                                            (ctypes.c_uint32 * (N + 1))(*range(N + 1)), (ctypes.c_uint32 * N)(*([0] * N))))

    def rand32():
        return bytes(rng.integers(0, 256, 32, dtype=np.uint8))

    def header(k, nparents):
        parents = [rand32() for _ in range(nparents)]
        hid = mr.header_id(pks[k], 5, [], parents)
        return mr.enc_header(pks[k], 5, [], parents, hid, orc.sign(seeds[k], hid)), hid

    def certificate(k):
        hdr, hid = header(k, 2)
        cd = mr.digest72(hid, 5, pks[k])
        voters = rng.permutation(N)[:67]
        return mr.msg_certificate(hdr, [(pks[v], orc.sign(seeds[v], cd)) for v in voters])

    def vote(k):
        hid, origin = rand32(), pks[(k + 1) % N]
        return mr.msg_vote(hid, 5, origin, pks[k], orc.sign(seeds[k], mr.digest72(hid, 5, origin)))

    pools = {"certificate": [certificate(k % N) for k in range(POOL)],
             "header": [mr.msg_header(header(k % N, 67)[0]) for k in range(POOL)],
             "vote": [vote(k % N) for k in range(POOL)]}
    pools["mix"] = [pools[("certificate", "header", "vote")[k % 3]][k // 3] for k in range(POOL)]
    res["message_bytes"] = {leg: sorted({len(b) for b in p})[-1] for leg, p in pools.items()}

    class Msgs:
        """a pool as C buffers: message k at ptr[k], len[k]; offs[k] = (0, len) for the batch entry"""

        def __init__(self, msgs):
            self.keep = [ctypes.create_string_buffer(b, len(b)) for b in msgs]
            self.ptr = [ctypes.addressof(b) for b in self.keep]
            self.len = [len(b) for b in msgs]
            self.offs = [(ctypes.c_uint64 * 2)(0, len(b)) for b in msgs]

    def route_a(h, ms, k, code):
        rc = lib.nwc_sanitize_messages(ms.ptr[k], ms.offs[k], 1, 0, None, code, None, None)
        return rc if rc < 0 else code[0]

    def route_b(h, ms, k, code):
        return lib.nwc_sanitizer_sanitize(h, ms.ptr[k], ms.len[k], 0, None, None, None)

    def check_invalid(h, msgs):
        """the pool's first message with a signature byte flipped: InvalidSignature on both routes"""
        b = bytearray(msgs[0])
        b[-20] ^= 1   # the last signature's s
        ms = Msgs([bytes(b)])
        for fn in (route_a, route_b):
            code = (ctypes.c_int32 * 1)()
            rc = fn(h, ms, 0, code)
            assert rc == 1, (fn.__name__, rc)

    def run_round(fn, h, T, ms):
        barrier = threading.Barrier(T + 1)
        out = [None] * T
        n = len(ms.ptr)

        def work(t):
            ts = []
            pc = time.perf_counter
            code = (ctypes.c_int32 * 1)()
            barrier.wait()
            t_start = pc()
            deadline = t_start + args.seconds
            k = t * (n // 16)
            while True:
                t0 = pc()
                rc = fn(h, ms, k % n, code)
                t1 = pc()
                ts.append(t1 - t0)
                if rc != 0:
                    out[t] = ("rc", rc)
                    return
                k += 1
                if t1 >= deadline:
                    break
            out[t] = (ts, pc() - t_start)

        ws = [threading.Thread(target=work, args=(t,)) for t in range(T)]
        for w in ws:
            w.start()
        barrier.wait()
        for w in ws:
            w.join()
        assert all(isinstance(o[0], list) for o in out), out
        lat = [x for o in out for x in o[0]]
        return len(lat), max(o[1] for o in out), lat

    def sstats(h):
        st = (ctypes.c_uint64 * 8)()
        assert lib.nwc_sanitizer_stats(h, st) == 0
        return [int(x) for x in st]

    def measure(leg, T, ms):
        h = lib.nwc_sanitizer_create(0, 0)
        assert h, lib.nwc_last_error()
        fns = {"A": route_a, "B": route_b}
        rows = {name: {"fn": fns[name], "calls": 0, "secs": 0.0, "lat": [], "round_rate": [], "round_p50": []}
                for name in args.route}
        st0 = None
        for rnd in range(args.rounds + 1):
            if rnd == 1:
                st0 = sstats(h)   # after the warm-up round
            for name, r in rows.items():
                calls, secs, lat = run_round(r["fn"], h, T, ms)
                if rnd:
                    r["calls"] += calls
                    r["secs"] += secs
                    r["lat"] += lat
                    r["round_rate"].append(calls / secs)
                    r["round_p50"].append(pct(lat, 0.5))
        st1 = sstats(h)
        assert lib.nwc_sanitizer_destroy(h) == 0
        out = {"threads": T}
        for name, r in rows.items():
            out[name] = {"calls_per_s": r["calls"] / r["secs"], "round_calls_per_s": r["round_rate"],
                         "round_calls_per_s_spread": max(r["round_rate"]) - min(r["round_rate"]),
                         "p50_us": pct(r["lat"], 0.5) * 1e6, "p99_us": pct(r["lat"], 0.99) * 1e6,
                         "round_p50_spread_us": (max(r["round_p50"]) - min(r["round_p50"])) * 1e6, "calls": r["calls"]}
        if "B" in out:
            d = [b - a for a, b in zip(st0, st1)]
            out["B"]["messages_per_group"] = d[1] / max(1, d[0])
            out["B"]["stats_delta"] = dict(zip(STATS[:6], d[:6]))
            out["B"]["max_messages_in_group"] = st1[6]
        if len(rows) == 2:
            out["B_over_A"] = out["B"]["calls_per_s"] / out["A"]["calls_per_s"]
        print(json.dumps({"leg": leg, **{k: (v if not isinstance(v, dict) else
                                             {kk: vv for kk, vv in v.items() if kk not in ("round_calls_per_s", "stats_delta")})
                                          for k, v in out.items()}}), flush=True)
        return out

    for leg in args.legs.split(","):
        ms = Msgs(pools[leg])
        hv = lib.nwc_sanitizer_create(0, 0)
        assert hv, lib.nwc_last_error()
        check_invalid(hv, pools[leg])
        lib.nwc_sanitizer_destroy(hv)
        res["legs"][leg] = [measure(leg, T, ms) for T in threads]
    _lib.check(lib.nwc_set_committee(None, 0))

    def row(leg, T):
        return next(r for r in res["legs"][leg] if r["threads"] == T)
    res["summary"] = {}
    for leg in res["legs"] if args.route == "AB" else ():
        tmax, tmin = max(threads), min(threads)
        hi, lo = row(leg, tmax), row(leg, tmin)
        spread = max(hi["A"]["round_calls_per_s_spread"], hi["B"]["round_calls_per_s_spread"])
        res["summary"][leg] = {
            "threads_max": tmax, "A_calls_per_s_at_max": hi["A"]["calls_per_s"], "B_calls_per_s_at_max": hi["B"]["calls_per_s"],
            "B_over_A_at_max": hi["B_over_A"], "larger_round_spread_at_max": spread,
            "B_beats_A_beyond_spread_at_max": hi["B"]["calls_per_s"] - hi["A"]["calls_per_s"] > spread,
            "messages_per_group_at_max": hi["B"]["messages_per_group"],
            "threads_min": tmin, "p50_us_A_at_min": lo["A"]["p50_us"], "p50_us_B_at_min": lo["B"]["p50_us"],
            "A_round_p50_spread_us_at_min": lo["A"]["round_p50_spread_us"],
            "B_p50_within_A_spread_at_min": lo["B"]["p50_us"] - lo["A"]["p50_us"] <= lo["A"]["round_p50_spread_us"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
