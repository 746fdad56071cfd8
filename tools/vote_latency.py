#!/usr/bin/env python3
"""Latency of making a vote for a sanitized header on an MI355X: the route a node has without
nwc_sanitizer_sanitize_vote against the vote fused into the sanitizer's group flight.

    python tools/vote_latency.py [--out profiles/vote/vote_latency.json]
    python tools/vote_latency.py --ab abtest/libnwc_parent.so [--out profiles/vote/plain_ab.json]

Method.  The message is a valid header of 67 parents from a committee of 100; the sanitizer is
created with (0, 0), so a lone caller launches at once and a burst shares what arrived together.
Route (a): nwc_sanitizer_sanitize, then Vote::digest with hashlib, then nwc_signer_sign.  Route (b):
nwc_sanitizer_sanitize_vote.  Wall clock (perf_counter) around each whole route, which ends with
the signature in host memory.  The two routes alternate in rounds (after a warm-up round of each);
p50 / p99 over all timed calls of a route, spread = max - min of the per-round p50s.  One thread:
--calls calls per route.  16 threads: bursts of 16 distinct headers released by a barrier, one per
thread, --calls calls per route in all; a call's time runs from its thread's release to its return,
a burst's from the release to the last return.  Every signature of both routes is compared with
the C restatement of dalek before anything is timed, and the two routes' with each other after.
--ab: the untouched path.  Lone-header p50 of plain nwc_sanitizer_sanitize in child processes that
load the parent commit's library and this build's (NWC_LIB_PATH) in the order A B B A, --ab-rounds
times each; rounds are compared within the state a process landed in (see ab()), and the allowed
margin is the spread of the parent's rounds of that state against each other.
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def summary(ts):
    return {"p50_us": pct(ts, 0.5) * 1e6, "p99_us": pct(ts, 0.99) * 1e6, "calls": len(ts)}


def world(n_committee, n_headers, parents):
    import numpy as np
    import messages_ref as mr
    from tests.oracle_lib import load_oracle
    orc = load_oracle()
    rng = np.random.default_rng(2027)
    r32 = lambda: bytes(rng.integers(0, 256, 32, dtype=np.uint8))   # noqa: E731
    seeds = [r32() for _ in range(n_committee)]
    pks = [orc.public_key(s) for s in seeds]
    hdrs = []
    for k in range(n_headers):
        ps = [r32() for _ in range(parents)]
        hid = mr.header_id(pks[k], 5 + k, [], ps)
        wire = mr.msg_header(mr.enc_header(pks[k], 5 + k, [], ps, hid, orc.sign(seeds[k], hid)))
        hdrs.append((wire, hid, 5 + k, pks[k]))
    return orc, pks, hdrs


def install(lib, pks):
    import ctypes
    from narwhal_amd import _lib
    n = len(pks)
    _lib.check(lib.nwc_set_committee_config(_lib.buf(b"".join(pks)), (ctypes.c_uint64 * n)(*([1] * n)), n,
                                            (ctypes.c_uint32 * (n + 1))(*range(n + 1)), (ctypes.c_uint32 * n)(*([0] * n))))


def plain_child(args):
    """One process, one library: lone-header latency of plain nwc_sanitizer_sanitize."""
    import ctypes
    from narwhal_amd import _lib
    lib = _lib.load()
    orc, pks, hdrs = world(100, 1, 67)
    install(lib, pks)
    wire, hid, rnd, author = hdrs[0]
    h = lib.nwc_sanitizer_create(0, 0)
    assert h, lib.nwc_last_error()
    dig, kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
    ts = []
    for i in range(args.calls + args.calls // 10):
        t0 = time.perf_counter()
        rc = lib.nwc_sanitizer_sanitize(h, _lib.buf(wire), len(wire), 0, None, dig, kind)
        ts.append(time.perf_counter() - t0)
        assert rc == 0 and dig.raw == hid
    assert lib.nwc_sanitizer_destroy(h) == 0
    print(json.dumps(dict(summary(ts[args.calls // 10:]), build_id=lib.nwc_build_id().decode())))


def ab(args):
    """Processes on one GPU were seen to land in one of two states in turn (a lone header's p50 at
    ~208 or ~228 us whatever the library), so the two libraries run in the order A B B A: each
    meets both states, and rounds are compared state by state."""
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
    both = p + t
    cut = (min(both) + max(both)) / 2 if max(both) - min(both) > 0.03 * min(both) else float("inf")
    res = {"what": "lone-header p50 of nwc_sanitizer_sanitize, header of 67 parents, committee of 100", "order": order,
           "rounds": rows, "parent_p50s_us": p, "this_p50s_us": t, "two_states": cut != float("inf"), "states": {}}
    ok = True
    for state, keep in (("fast", lambda x: x < cut), ("slow", lambda x: x >= cut)):
        ps, ts = [x for x in p if keep(x)], [x for x in t if keep(x)]
        if not ps or not ts:
            continue
        st = {"parent_p50_us": pct(ps, 0.5), "this_p50_us": pct(ts, 0.5), "parent_spread_us": max(ps) - min(ps),
              "parent_rounds": len(ps), "this_rounds": len(ts)}
        st["this_minus_parent_us"] = min(ts) - min(ps) if len(ps) < 2 else pct(ts, 0.5) - pct(ps, 0.5)
        st["within_margin"] = st["this_minus_parent_us"] <= st["parent_spread_us"]
        ok = ok and st["within_margin"]
        res["states"][state] = st
    res["within_margin"] = ok
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab", default=None, help="the parent commit's library, relative to the repository root")
    ap.add_argument("--ab-rounds", type=int, default=6)
    ap.add_argument("--plain-child", action="store_true")
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    if args.ab:
        res = ab(args)
        out = args.out or os.path.join(ROOT, "profiles", "vote", "plain_ab.json")
    else:
        res = routes(args)
        out = args.out or os.path.join(ROOT, "profiles", "vote", "vote_latency.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}))


def routes(args):
    import ctypes
    import torch
    from narwhal_amd import _lib
    from narwhal_amd import build as nb
    assert torch.cuda.is_available(), "vote_latency.py measures on a GPU"
    lib = _lib.load()
    T = 16
    orc, pks, hdrs = world(100, T, 67)
    install(lib, pks)
    seed = bytes(range(1, 33))
    signer = lib.nwc_signer_create(_lib.buf(seed + orc.public_key(seed)))
    assert signer, lib.nwc_last_error()
    san = lib.nwc_sanitizer_create(0, 0)
    assert san, lib.nwc_last_error()
    want = [orc.sign(seed, hashlib.sha512(hid + struct.pack("<Q", rnd) + author).digest()[:32]) for _, hid, rnd, author in hdrs]

    class Ctx:   # one thread's buffers
        def __init__(self):
            self.dig, self.kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
            self.sig, self.voted = ctypes.create_string_buffer(64), ctypes.c_int32(0)

    def route_a(c, k):
        wire, hid, rnd, author = hdrs[k]
        rc = lib.nwc_sanitizer_sanitize(san, _lib.buf(wire), len(wire), 0, None, c.dig, c.kind)
        assert rc == 0
        d = hashlib.sha512(c.dig.raw + struct.pack("<Q", rnd) + author).digest()[:32]
        assert lib.nwc_signer_sign(signer, _lib.buf(d), c.sig) == 0

    def route_b(c, k):
        wire = hdrs[k][0]
        rc = lib.nwc_sanitizer_sanitize_vote(san, signer, _lib.buf(wire), len(wire), 0, None, c.dig, c.kind, c.sig,
                                             ctypes.byref(c.voted))
        assert rc == 0 and c.voted.value == 1

    c0 = Ctx()
    for k in range(T):
        for route in (route_a, route_b):
            route(c0, k)
            assert c0.sig.raw == want[k], (route.__name__, k)

    res = {"build_id": lib.nwc_build_id().decode(), "sources": nb.source_id(), "device": torch.cuda.get_device_name(0),
           "method": __doc__.split("Method.")[1].strip().replace("\n", " "), "rounds": args.rounds}
    names = {"a": route_a, "b": route_b}

    # ---- one thread
    per_round = max(1, args.calls // args.rounds)
    times = {"a": [], "b": []}
    p50s = {"a": [], "b": []}
    for rnd in range(args.rounds + 1):
        for name, route in names.items():
            ts = []
            for i in range(per_round if rnd else max(100, per_round // 10)):
                t0 = time.perf_counter()
                route(c0, 0)
                ts.append(time.perf_counter() - t0)
            assert c0.sig.raw == want[0]
            if rnd:
                times[name] += ts
                p50s[name].append(pct(ts, 0.5))
    one = {n: dict(summary(times[n]), round_p50_spread_us=(max(p50s[n]) - min(p50s[n])) * 1e6) for n in names}
    one["b_minus_a_p50_us"] = one["b"]["p50_us"] - one["a"]["p50_us"]
    res["threads_1"] = one
    print(json.dumps(one), flush=True)

    # ---- 16 threads, bursts of 16 distinct headers
    bursts = max(1, args.calls // T // args.rounds)
    plan = [(rnd, name) for rnd in range(args.rounds + 1) for name in names]
    start = threading.Barrier(T + 1)
    done = threading.Barrier(T + 1)
    call_t = {(rnd, name): [] for rnd, name in plan}
    lock = threading.Lock()

    def count(rnd):
        return bursts if rnd else max(10, bursts // 10)

    def worker(k):
        c = Ctx()
        for rnd, name in plan:
            mine = []
            for _ in range(count(rnd)):
                start.wait()
                t0 = time.perf_counter()
                names[name](c, k)
                mine.append(time.perf_counter() - t0)
                assert c.sig.raw == want[k]
                done.wait()
            with lock:
                call_t[(rnd, name)] += mine
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(T)]
    for t in threads:
        t.start()
    burst_t = {(rnd, name): [] for rnd, name in plan}
    vs0 = (ctypes.c_uint64(0), ctypes.c_uint64(0))
    for rnd, name in plan:
        for _ in range(count(rnd)):
            start.wait()
            t0 = time.perf_counter()
            done.wait()
            burst_t[(rnd, name)].append(time.perf_counter() - t0)
    for t in threads:
        t.join()
    many = {}
    for name in names:
        calls = [x for rnd in range(1, args.rounds + 1) for x in call_t[(rnd, name)]]
        bs = [x for rnd in range(1, args.rounds + 1) for x in burst_t[(rnd, name)]]
        rp = [pct(call_t[(rnd, name)], 0.5) for rnd in range(1, args.rounds + 1)]
        many[name] = dict(summary(calls), round_p50_spread_us=(max(rp) - min(rp)) * 1e6, burst_p50_us=pct(bs, 0.5) * 1e6,
                          burst_p99_us=pct(bs, 0.99) * 1e6)
    many["b_minus_a_p50_us"] = many["b"]["p50_us"] - many["a"]["p50_us"]
    many["b_minus_a_burst_p50_us"] = many["b"]["burst_p50_us"] - many["a"]["burst_p50_us"]
    res["threads_16"] = many
    print(json.dumps(many), flush=True)

    st = (ctypes.c_uint64 * 8)()
    assert lib.nwc_sanitizer_stats(san, st) == 0
    assert lib.nwc_sanitizer_vote_stats(san, ctypes.byref(vs0[0]), ctypes.byref(vs0[1])) == 0
    res["sanitizer"] = {"groups": int(st[0]), "messages": int(st[1]), "redone_messages": int(st[4]),
                        "max_messages_in_group": int(st[6]), "votes_in_flight": int(vs0[0].value), "votes_alone": int(vs0[1].value)}
    assert lib.nwc_sanitizer_destroy(san) == 0 and lib.nwc_signer_destroy(signer) == 0
    return res


if __name__ == "__main__":
    main()
