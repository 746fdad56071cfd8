#!/usr/bin/env python3
"""Signing rates and latencies on an MI355X: the registered-key signer (k_sign, k_sign_wide) against
the workload generator it replaces for signing (k_keygen_sign, which re-derives the key per lane)
and against the CPU oracle.

    python tools/sign_rate.py [--out profiles/sign/sign_rate.json]

Method.  Call latency: wall clock (perf_counter) around nwc_signer_sign_many of n host digests --
the call returns with the signatures in host memory, so it ends in a device wait; the lane and the
wide kernel alternate in rounds of --calls calls each (after a warm-up round), p50 / p99 over all
timed calls of a path, and the spread = max - min of the per-round p50s of that path.  The suggested
NWC_SIGN_WIDE_MAX is the largest n of the sweep at which p50(wide) + max(spread) < p50(lane), 0 if
none.  Throughput: device events around nwc_dev_sign of 1,048,576 device-resident digests, median
of --reps launches after a warm-up.  Parent paths on the same digests: device.keygen_sign_host at
n = 1 (seed upload, k_keygen_sign, download) and device.keygen_sign at 1,048,576.  Host baseline:
orc_keygen_sign_many (keygen + sign per item, the oracle's only bulk signing entry) on 1 and on
16 threads.  Every GPU result is checked against the oracle before it is timed.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign", "sign_rate.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=1 << 20)
    ap.add_argument("--sweep", default="1,2,4,8,16,32,64,128,256,1024")
    args = ap.parse_args()
    import numpy as np
    import torch
    from narwhal_amd import _lib, crypto, device
    from narwhal_amd import build as nb
    from tests.oracle_lib import load_oracle
    assert torch.cuda.is_available(), "sign_rate.py measures on a GPU"
    lib = _lib.load()
    orc = load_oracle()
    seed = bytes(range(1, 33))
    pk = orc.public_key(seed)
    signer = crypto.Signer(seed + pk)
    rng = np.random.default_rng(2026)
    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "),
           "calls_per_round": args.calls, "rounds": args.rounds}

    # ---- call latency, lane vs wide, alternating rounds
    def host_call(d, out):
        return lib.nwc_signer_sign_many(signer.handle, _lib.buf(d), d.shape[0], _lib.buf(out))

    sweep = []
    for n in [int(x) for x in args.sweep.split(",")]:
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        out = np.zeros((n, 64), np.uint8)
        exp = np.stack([np.frombuffer(orc.sign(seed, d[i].tobytes()), np.uint8) for i in range(min(n, 8))])
        times = {1: [], 2: []}
        p50s = {1: [], 2: []}
        for rnd in range(args.rounds + 1):
            for path in (1, 2):
                _lib.diag_set("sign_path", path)
                ts = []
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    rc = host_call(d, out)
                    ts.append(time.perf_counter() - t0)
                    assert rc == 0
                assert (out[:exp.shape[0]] == exp).all()
                if rnd:   # round 0 warms up
                    times[path] += ts
                    p50s[path].append(pct(ts, 0.5))
        row = {"n": n}
        for path, name in ((1, "lane"), (2, "wide")):
            row[name] = {"p50_us": pct(times[path], 0.5) * 1e6, "p99_us": pct(times[path], 0.99) * 1e6,
                         "round_p50_spread_us": (max(p50s[path]) - min(p50s[path])) * 1e6}
        spread = max(row["lane"]["round_p50_spread_us"], row["wide"]["round_p50_spread_us"])
        row["wide_wins"] = row["wide"]["p50_us"] + spread < row["lane"]["p50_us"]
        sweep.append(row)
        print(json.dumps(row), flush=True)
    _lib.diag_set("sign_path", 0)
    res["call_latency"] = sweep
    res["suggested_sign_wide_max"] = max([r["n"] for r in sweep if r["wide_wins"]], default=0)

    # ---- device-resident throughput
    n = args.big
    msgs = device.derive32(b"sign-rate-msg", 0, n)
    seeds = torch.from_numpy(np.tile(np.frombuffer(seed, np.uint8), (n, 1))).cuda()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return r, sorted(ms)[len(ms) // 2], ms

    _lib.diag_set("sign_path", 1)
    sigs, ms_new, all_new = timed(lambda: device.sign(signer, msgs))
    _lib.diag_set("sign_path", 0)
    (_, sigs_old), ms_old, all_old = timed(lambda: device.keygen_sign(seeds, msgs))
    assert torch.equal(sigs, sigs_old), "signer and k_keygen_sign disagree"
    hm = msgs[:64].cpu().numpy()
    assert all(sigs[i].cpu().numpy().tobytes() == orc.sign(seed, hm[i].tobytes()) for i in range(64))
    res["device_resident"] = {"n": n, "k_sign": {"ms_median": ms_new, "ms_all": all_new, "signatures_per_s": n / ms_new * 1e3},
                              "parent_k_keygen_sign": {"ms_median": ms_old, "ms_all": all_old,
                                                       "signatures_per_s": n / ms_old * 1e3}}
    print(json.dumps(res["device_resident"]), flush=True)

    # ---- parent path at n = 1 (the mirror's Signature.new route)
    d1 = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    ts = []
    for i in range(args.calls + 20):
        t0 = time.perf_counter()
        _, sg = device.keygen_sign_host(seed, d1, 1)
        ts.append(time.perf_counter() - t0)
    assert sg == orc.sign(seed, d1)
    ts = ts[20:]
    res["parent_keygen_sign_host_n1"] = {"p50_us": pct(ts, 0.5) * 1e6, "p99_us": pct(ts, 0.99) * 1e6}
    print(json.dumps(res["parent_keygen_sign_host_n1"]), flush=True)

    # ---- host baseline
    host = {}
    for threads, cnt in ((1, 20000), (16, 320000)):
        hs = np.tile(np.frombuffer(seed, np.uint8), (cnt, 1))
        hd = rng.integers(0, 256, (cnt, 32), dtype=np.uint8)
        orc.keygen_sign_many(hs[:1000], hd[:1000], threads=threads)
        t0 = time.perf_counter()
        orc.keygen_sign_many(hs, hd, threads=threads)
        dt = time.perf_counter() - t0
        host["threads_%d" % threads] = {"n": cnt, "signatures_per_s": cnt / dt, "us_per_signature_per_thread": dt / cnt * threads * 1e6}
    res["host_orc_keygen_sign_many"] = host
    print(json.dumps(host), flush=True)

    one = next(r for r in sweep if r["n"] == 1)
    res["ratios"] = {
        "n1_call_p50_parent_over_lane": res["parent_keygen_sign_host_n1"]["p50_us"] / one["lane"]["p50_us"],
        "n1_call_p50_parent_over_wide": res["parent_keygen_sign_host_n1"]["p50_us"] / one["wide"]["p50_us"],
        "n1_call_p50_lane_over_host_core": one["lane"]["p50_us"] / host["threads_1"]["us_per_signature_per_thread"],
        "big_k_sign_over_parent": ms_old / ms_new,
        "big_k_sign_over_host_1_thread": (n / ms_new * 1e3) / host["threads_1"]["signatures_per_s"],
        "big_k_sign_over_host_16_threads": (n / ms_new * 1e3) / host["threads_16"]["signatures_per_s"],
    }
    signer.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["ratios"]))


if __name__ == "__main__":
    main()
