#!/usr/bin/env python3
"""Small verify calls from many threads on an MI355X: nwc_verify_batch (one call at a time per
device) against a verifier (nwc_verifier: concurrent calls share a launch), same binary.

    python tools/verifier_rate.py [--out profiles/verifier/verifier_rate.json]

Method.  One process, T = 1, 2, 4, 8, 16 Python threads (ctypes releases the GIL around a call;
never more than 16 threads).  Every call verifies one config-1 certificate: 3 votes of a 4-key
committee over its own digest.  Three legs: "committee" = the keys cached through
nwc_set_committee; "auto" = no committee, the auto key cache warm (every certificate seen twice
before timing); "first_sight" = no committee and fresh keys in every call (generated on the GPU
beforehand, each certificate used once).  For every leg and T, rounds alternate between route A =
nwc_verify_batch and route B = nwc_verifier_verify_batch on one verifier created with (0, 0):
--rounds timed rounds of --seconds each after one warm-up round of both.  A round starts all
threads at a barrier; each thread calls back to back until the round's time is up and times
every call with perf_counter.  Reported per leg, T and route: calls/s over all timed rounds, the
per-round calls/s and their spread (max - min), p50 / p99 of the per-call latency over all timed
calls, the spread of the per-round p50s, and for B the mean requests per group (from
nwc_verifier_stats).  Every answer is checked (all certificates are valid; one corrupted
certificate per leg must come back invalid with the right bad vote on both routes).  The Python
loop costs a few microseconds per call under the GIL, which bounds what 16 threads can show.
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

CPU_PORT_CALLS_PER_S = 126.9e3   # the 16-thread CPU port on config 1


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier", "verifier_rate.json"))
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", default="1,2,4,8,16")
    ap.add_argument("--legs", default="committee,auto,first_sight")
    ap.add_argument("--pool", type=int, default=1 << 20, help="fresh certificates generated per T of the first-sight leg")
    args = ap.parse_args()
    import numpy as np
    import torch
    from narwhal_amd import _lib, device
    from narwhal_amd import build as nb
    from tests.oracle_lib import load_oracle
    assert torch.cuda.is_available(), "verifier_rate.py measures on a GPU"
    threads = [int(x) for x in args.threads.split(",")]
    assert max(threads) <= 16
    lib = _lib.load()
    orc = load_oracle()
    rng = np.random.default_rng(2026)
    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "), "seconds_per_round": args.seconds,
           "rounds": args.rounds, "cpu_port_16_threads_calls_per_s": CPU_PORT_CALLS_PER_S, "legs": {}}

    # the committee's certificates: 64 per thread, votes of 3 of the 4 keys over each digest
    seeds = [bytes([k + 1]) * 32 for k in range(4)]
    keys = np.stack([np.frombuffer(orc.public_key(s), np.uint8) for s in seeds])
    ncert = 16 * 64
    cm = rng.integers(0, 256, (ncert, 32), dtype=np.uint8)
    cp = np.zeros((ncert, 3, 32), np.uint8)
    cs = np.zeros((ncert, 3, 64), np.uint8)
    for c in range(ncert):
        for j, k in enumerate(sorted(rng.choice(4, 3, replace=False))):
            cp[c, j] = keys[k]
            cs[c, j] = np.frombuffer(orc.sign(seeds[k], cm[c].tobytes()), np.uint8)

    def route_a(h, m, p, s, bm):
        return lib.nwc_verify_batch(m, p, s, 3, bm)

    def route_b(h, m, p, s, bm):
        return lib.nwc_verifier_verify_batch(h, m, p, s, 3, bm)

    def check_invalid(h, m, p, s):
        """a certificate with vote 1 corrupted: invalid with bad set {1} on both routes"""
        bad = s.copy()
        bad[1, 40] ^= 1
        for fn in (route_a, route_b):
            bm = np.zeros(1, np.uint8)
            rc = fn(h, m.ctypes.data, p.ctypes.data, bad.ctypes.data, bm.ctypes.data)
            assert rc == 1 and bm[0] == 2, (fn.__name__, rc, bm)

    def run_round(fn, h, T, m, p, s, first, per_thread, reuse):
        """T threads; thread t calls on certificates first + t * per_thread + (0, 1, ...), wrapping only
        if reuse; returns (calls, seconds, latencies)"""
        mb, pb, sb = m.ctypes.data, p.ctypes.data, s.ctypes.data
        barrier = threading.Barrier(T + 1)
        out = [None] * T

        def work(t):
            ts = []
            pc = time.perf_counter
            lo = first + t * per_thread
            barrier.wait()
            t_start = pc()
            deadline = t_start + args.seconds
            k = 0
            while True:
                i = lo + (k % per_thread if reuse else k)
                t0 = pc()
                rc = fn(h, mb + 32 * i, pb + 96 * i, sb + 192 * i, None)
                t1 = pc()
                ts.append(t1 - t0)
                if rc != 0:
                    out[t] = ("rc", rc)
                    return
                k += 1
                if t1 >= deadline or (not reuse and k == per_thread):
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

    def vstats(h):
        st = (ctypes.c_uint64 * 8)()
        assert lib.nwc_verifier_stats(h, st) == 0
        return [int(x) for x in st]

    def measure(leg, T, m, p, s, reuse, per_thread):
        h = lib.nwc_verifier_create(0, 0)
        assert h, lib.nwc_last_error()
        rows = {"A": {"fn": route_a, "calls": 0, "secs": 0.0, "lat": [], "round_rate": [], "round_p50": []},
                "B": {"fn": route_b, "calls": 0, "secs": 0.0, "lat": [], "round_rate": [], "round_p50": []}}
        st0 = None
        slot = 0
        for rnd in range(args.rounds + 1):
            if rnd == 1:
                st0 = vstats(h)   # after the warm-up round
            for name in ("A", "B"):
                r = rows[name]
                first = 0 if reuse else slot * T * per_thread
                slot += 1
                calls, secs, lat = run_round(r["fn"], h, T, m, p, s, first, per_thread, reuse)
                if rnd:
                    r["calls"] += calls
                    r["secs"] += secs
                    r["lat"] += lat
                    r["round_rate"].append(calls / secs)
                    r["round_p50"].append(pct(lat, 0.5))
        st1 = vstats(h)
        assert lib.nwc_verifier_destroy(h) == 0
        out = {"threads": T}
        for name, r in rows.items():
            out[name] = {"calls_per_s": r["calls"] / r["secs"], "round_calls_per_s": r["round_rate"],
                         "round_calls_per_s_spread": max(r["round_rate"]) - min(r["round_rate"]),
                         "p50_us": pct(r["lat"], 0.5) * 1e6, "p99_us": pct(r["lat"], 0.99) * 1e6,
                         "round_p50_spread_us": (max(r["round_p50"]) - min(r["round_p50"])) * 1e6, "calls": r["calls"]}
        d = [b - a for a, b in zip(st0, st1)]
        out["B"]["requests_per_group"] = d[1] / max(1, d[0])
        out["B"]["stats_delta"] = dict(zip(("groups", "requests", "equations", "wide_equations", "cold_equations",
                                            "redone_equations", "bypassed_requests"), d[:7]))
        out["B_over_A"] = out["B"]["calls_per_s"] / out["A"]["calls_per_s"]
        print(json.dumps({"leg": leg, **{k: (v if not isinstance(v, dict) else
                                             {kk: vv for kk, vv in v.items() if kk not in ("round_calls_per_s", "stats_delta")})
                                          for k, v in out.items()}}), flush=True)
        return out

    for leg in args.legs.split(","):
        rows = []
        if leg == "committee":
            _lib.check(lib.nwc_set_committee(keys.ctypes.data, 4))
        else:
            _lib.check(lib.nwc_set_committee(None, 0))
        if leg in ("committee", "auto"):
            for c in range(ncert):   # two sightings: the auto leg's keys are in the auto cache from here on
                for _ in range(2):
                    assert route_a(None, cm[c].ctypes.data, cp[c].ctypes.data, cs[c].ctypes.data, None) == 0
            hv = lib.nwc_verifier_create(0, 0)
            check_invalid(hv, cm[5], cp[5], cs[5])
            lib.nwc_verifier_destroy(hv)
            for T in threads:
                rows.append(measure(leg, T, cm, cp, cs, True, 64))
        else:
            slots = 2 * (args.rounds + 1)
            for T in threads:
                n = args.pool
                msgs = device.derive32(b"vrate-msg-%d" % T, 0, n)
                vseeds = device.derive32(b"vrate-seed-%d" % T, 0, 3 * n)
                pks, sigs = device.keygen_sign(vseeds, msgs.repeat_interleave(3, dim=0))
                torch.cuda.synchronize()
                m, p, s = (x.cpu().numpy() for x in (msgs, pks, sigs))
                del msgs, vseeds, pks, sigs
                hv = lib.nwc_verifier_create(0, 0)
                check_invalid(hv, m[n - 1], p[3 * n - 3:].reshape(3, 32), s[3 * n - 3:].reshape(3, 64))
                lib.nwc_verifier_destroy(hv)
                rows.append(measure(leg, T, m, p, s, False, (n - 1) // (slots * T)))
        res["legs"][leg] = rows
    _lib.check(lib.nwc_set_committee(None, 0))

    def row(leg, T):
        return next(r for r in res["legs"][leg] if r["threads"] == T)
    res["summary"] = {}
    for leg in res["legs"]:
        tmax, tmin = max(threads), min(threads)
        hi, lo = row(leg, tmax), row(leg, tmin)
        res["summary"][leg] = {
            "threads_max": tmax, "B_over_A_at_max": hi["B_over_A"],
            "gain_calls_per_s_at_max": hi["B"]["calls_per_s"] - hi["A"]["calls_per_s"],
            "A_round_spread_at_max": hi["A"]["round_calls_per_s_spread"],
            "B_beats_A_beyond_spread_at_max": hi["B"]["calls_per_s"] - hi["A"]["calls_per_s"] > hi["A"]["round_calls_per_s_spread"],
            "threads_min": tmin, "p50_us_A_at_min": lo["A"]["p50_us"], "p50_us_B_at_min": lo["B"]["p50_us"],
            "A_round_p50_spread_us_at_min": lo["A"]["round_p50_spread_us"],
            "B_p50_within_A_spread_at_min": lo["B"]["p50_us"] - lo["A"]["p50_us"] <= lo["A"]["round_p50_spread_us"],
            "B_at_max_over_cpu_port": hi["B"]["calls_per_s"] / CPU_PORT_CALLS_PER_S}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
