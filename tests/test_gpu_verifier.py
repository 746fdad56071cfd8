"""GPU tests of nwc_verifier (include/nwc.h): concurrent small verify calls packed into groups that
share one launch of k_verify_group_wide / k_verify_group_cold, every equation under its own mode.

Verdicts are always compared with tests/golden/ or the CPU oracle (dalek verify_strict / the exact
batch leaf restated), never with the library alone.  Keys and signatures of random requests come
from the oracle as well.  Groups are made deterministic by max_requests: a verifier created with
(k, 5 s) launches exactly when its k-th request has arrived, and nwc_verifier_stats counts a request
the moment it joins a group, so a test can order arrivals without sleeping."""
import ctypes
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

STATS = ("groups", "requests", "equations", "wide_equations", "cold_equations", "redone_equations",
         "bypassed_requests", "max_requests_in_group")
LONG_WAIT_US = 5_000_000


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    lb = _lib.load()
    _lib.check(lb.nwc_set_committee(None, 0))
    return lb


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class V:
    """A verifier handle with numpy-friendly calls; destroyed on exit."""

    def __init__(self, lib, max_requests, max_wait_us):
        self.lib = lib
        self.h = lib.nwc_verifier_create(max_requests, max_wait_us)
        assert self.h, lib.nwc_last_error()

    def strict(self, m, p, s):
        m, p, s = (np.ascontiguousarray(x) for x in (m, p, s))
        rc = self.lib.nwc_verifier_verify_strict(self.h, _p(m), _p(p), _p(s))
        assert rc in (0, 1), (rc, self.lib.nwc_last_error())
        return rc == 0

    def batch(self, m, P, S):
        """(verdict, per-vote valid) of one certificate"""
        m, P, S = (np.ascontiguousarray(x) for x in (m, P, S))
        n = P.shape[0]
        bm = np.zeros((n + 7) // 8 or 1, np.uint8)
        rc = self.lib.nwc_verifier_verify_batch(self.h, _p(m), _p(P), _p(S), n, _p(bm))
        assert rc in (0, 1), (rc, self.lib.nwc_last_error())
        return rc == 0, ~np.unpackbits(bm, bitorder="little")[:n].astype(bool)

    def stats(self):
        out = (ctypes.c_uint64 * 8)()
        assert self.lib.nwc_verifier_stats(self.h, out) == 0
        return dict(zip(STATS, (int(x) for x in out)))

    def wait_requests(self, k):
        while self.stats()["requests"] < k:   # the k-th request has joined its group
            pass

    def close(self):
        if self.h:
            h, self.h = self.h, None
            assert self.lib.nwc_verifier_destroy(h) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _signed(oracle, seed, n, msgs=None):
    """n triples signed by the oracle with fresh keys; msgs: (n, 32) or one digest for all"""
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if msgs is None:
        msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    elif msgs.ndim == 1:
        msgs = np.tile(msgs, (n, 1))
    pks, sigs = oracle.keygen_sign_many(seeds, np.ascontiguousarray(msgs))
    return np.ascontiguousarray(msgs), pks, sigs


def _cert(oracle, seed, n):
    """a certificate: one digest, n votes"""
    digest = np.random.default_rng(seed + 7919).integers(0, 256, 32, dtype=np.uint8)
    _, pks, sigs = _signed(oracle, seed, n, digest)
    return digest, pks, sigs


def _ordered(pool, v, jobs):
    """start the jobs one after another, each once the previous one has joined its group"""
    base = v.stats()["requests"]
    futs = []
    for k, job in enumerate(jobs):
        futs.append(pool.submit(job))
        v.wait_requests(base + k + 1)
    return [f.result(timeout=60) for f in futs]


def test_deterministic_coalescing(lib, oracle):
    digest, pks, sigs = _cert(oracle, 1, 3)
    with V(lib, 8, 2_000_000) as v, ThreadPoolExecutor(8) as pool:
        futs = [pool.submit(v.batch, digest, pks, sigs) for _ in range(8)]
        assert all(f.result(timeout=60)[0] for f in futs)
        st = v.stats()
        assert (st["groups"], st["requests"], st["equations"], st["max_requests_in_group"]) == (1, 8, 24, 8), st
    with V(lib, 0, 0) as v:
        for k in range(5):
            ok, valid = v.batch(digest, pks, sigs)
            assert ok and valid.all()
            assert v.strict(digest, pks[0], sigs[0])
        st = v.stats()
        assert (st["groups"], st["requests"], st["max_requests_in_group"]) == (10, 10, 1), st   # each call its own group


def test_mode_per_equation(lib, golden_verify):
    """Every golden case with a 32-byte message as a strict request and as a one-vote batch request,
    in shared groups: each answer is the fixture's `strict` or `leaf` (they differ in 11 cases, so a
    launch-uniform mode fails)."""
    cases = [c for c in golden_verify["cases"] if len(c["msg"]) == 64]
    assert len(cases) == 130 and sum(c["strict"] != c["leaf"] for c in cases) == 11
    arr = lambda c, k: np.frombuffer(bytes.fromhex(c[k]), np.uint8)  # noqa: E731
    jobs = [(c, mode) for c in cases for mode in ("strict", "leaf")]
    np.random.default_rng(3).shuffle(jobs)
    with V(lib, 16, 500) as v, ThreadPoolExecutor(8) as pool:
        def run(job):
            c, mode = job
            m, p, s = arr(c, "msg"), arr(c, "pk"), arr(c, "sig")
            if mode == "strict":
                return v.strict(m, p, s)
            ok, valid = v.batch(m, p[None, :], s[None, :])
            assert ok == bool(valid[0])
            return ok
        got = list(pool.map(run, jobs))
        st = v.stats()
    wrong = [(c["name"], mode) for (c, mode), g in zip(jobs, got) if g != c[mode]]
    assert not wrong, wrong[:8]
    assert st["requests"] == 260 and st["groups"] < 260 and st["max_requests_in_group"] >= 2, st


def test_golden_batches_with_strict_traffic(lib, golden_verify, golden_batch):
    cases = [c for c in golden_verify["cases"] if len(c["msg"]) == 64][:44]
    assert len(golden_batch) == 22
    arr = lambda h: np.frombuffer(bytes.fromhex(h), np.uint8)  # noqa: E731
    jobs = []
    for k, b in enumerate(golden_batch):
        jobs += [("batch", b), ("strict", cases[2 * k]), ("strict", cases[2 * k + 1])]
    with V(lib, 16, 300) as v, ThreadPoolExecutor(8) as pool:
        def run(job):
            kind, x = job
            if kind == "strict":
                return v.strict(arr(x["msg"]), arr(x["pk"]), arr(x["sig"]))
            n = len(x["votes"])
            P = np.stack([arr(p) for p, _ in x["votes"]]) if n else np.zeros((0, 32), np.uint8)
            S = np.stack([arr(s) for _, s in x["votes"]]) if n else np.zeros((0, 64), np.uint8)
            ok, valid = v.batch(arr(x["msg"]), P, S)
            return ok, [int(i) for i in np.nonzero(~valid)[0]]
        got = list(pool.map(run, jobs))
    for (kind, x), g in zip(jobs, got):
        if kind == "strict":
            assert g == x["strict"], x["name"]
        else:
            assert g == (x["verdict"], x["bad"]), (x["name"], g)


def test_both_kernels_in_one_group(lib, oracle):
    from narwhal_amd import _lib
    _lib.check(lib.nwc_set_committee(None, 0))   # no committee, and an empty auto cache
    warm = _cert(oracle, 21, 3)
    fresh = _cert(oracle, 22, 3)
    with V(lib, 2, LONG_WAIT_US) as v, ThreadPoolExecutor(2) as pool:
        with V(lib, 0, 0) as solo:
            for _ in range(2):   # two sightings put the keys into the auto cache
                assert solo.batch(*warm)[0]
            before = solo.stats()
            assert before["cold_equations"] == 6 and before["wide_equations"] == 0, before
            assert solo.batch(*warm)[0]
            assert solo.stats()["wide_equations"] == 3
        bad = fresh[2].copy()
        bad[1, 5] ^= 4
        (ok_w, valid_w), (ok_f, valid_f) = _ordered(pool, v, [lambda: v.batch(*warm), lambda: v.batch(fresh[0], fresh[1], bad)])
        st = v.stats()
        assert (st["groups"], st["wide_equations"], st["cold_equations"]) == (1, 3, 3), st
        assert ok_w and (valid_w == oracle.leaf_many(np.tile(warm[0], (3, 1)), warm[1], warm[2])).all()
        assert not ok_f and (valid_f == oracle.leaf_many(np.tile(fresh[0], (3, 1)), fresh[1], bad)).all()
        assert list(valid_f) == [True, False, True]
    # a committee of 4 keys and one request whose key is outside it
    com = _cert(oracle, 23, 4)
    out_m, out_p, out_s = _signed(oracle, 24, 1)
    _lib.check(lib.nwc_set_committee(_p(np.ascontiguousarray(com[1])), 4))
    try:
        with V(lib, 2, LONG_WAIT_US) as v, ThreadPoolExecutor(2) as pool:
            (ok_c, valid_c), ok_o = _ordered(pool, v, [lambda: v.batch(com[0], com[1][:3], com[2][:3]),
                                                       lambda: v.strict(out_m[0], out_p[0], out_s[0])])
            st = v.stats()
            assert (st["groups"], st["wide_equations"], st["cold_equations"]) == (1, 3, 1), st
            assert ok_c and valid_c.all() and oracle.leaf_many(np.tile(com[0], (3, 1)), com[1][:3], com[2][:3]).all()
            assert ok_o and oracle.strict_many(out_m, out_p, out_s)[0]
    finally:
        _lib.check(lib.nwc_set_committee(None, 0))


def test_bit_placement_off_a_word_boundary(lib, oracle):
    """A 67-vote certificate as the third request of a group (its equations start at 6, off every
    64 boundary) with votes 0, 63, 64 and 66 corrupted: the bad bitmap is the oracle's and the
    neighbours' answers are untouched."""
    a, b = _cert(oracle, 31, 3), _cert(oracle, 32, 3)
    digest, pks, sigs = _cert(oracle, 33, 67)
    for i in (0, 63, 64, 66):
        sigs[i, 40] ^= 1
    with V(lib, 3, LONG_WAIT_US) as v, ThreadPoolExecutor(3) as pool:
        ra, rb, rc = _ordered(pool, v, [lambda: v.batch(*a), lambda: v.batch(*b), lambda: v.batch(digest, pks, sigs)])
        st = v.stats()
    assert (st["groups"], st["requests"], st["equations"]) == (1, 3, 73), st
    exp = oracle.leaf_many(np.tile(digest, (67, 1)), pks, sigs)
    assert list(np.nonzero(~exp)[0]) == [0, 63, 64, 66]
    assert not rc[0] and (rc[1] == exp).all()
    assert ra[0] and ra[1].all() and rb[0] and rb[1].all()


def test_redo_path():
    """NWC_FORCE_FALLBACK_EVERY=3 in a child process: every third first-sight equation of a group asks
    to be decided again; 200 mixed requests still equal the oracle in both modes."""
    env = dict(os.environ, NWC_FORCE_FALLBACK_EVERY="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "verifier_fallback_helper.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["requests"] == 200 and out["mismatches"] == 0, out
    assert out["stats"]["redone_equations"] > 0 and out["stats"]["requests"] == 200, out
    assert out["strict_requests"] > 20 and out["batch_requests"] > 20 and out["invalid"] > 10, out


def _random_requests(oracle, seed, count, max_votes):
    """requests of 1..max_votes votes (single votes are strict half the time), a fifth corrupted in
    s, R, the message or the key"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, max_votes + 1, count)
    sizes[rng.random(count) < 0.3] = 1
    reqs = []
    for k, n in enumerate(sizes):
        digest, pks, sigs = _cert(oracle, seed * 100003 + k, int(n))
        digest, pks, sigs = digest.copy(), pks.copy(), sigs.copy()
        if rng.random() < 0.2:
            i = int(rng.integers(0, n))
            what = int(rng.integers(0, 4))
            if what == 0:
                sigs[i, 32 + rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)   # s
            elif what == 1:
                sigs[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)        # R
            elif what == 2:
                digest[rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)         # the message
            else:
                pks[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)         # the key
        reqs.append((bool(n == 1 and rng.random() < 0.5), digest, pks, sigs))
    return reqs


def test_equal_to_the_parent_route(lib, oracle):
    reqs = _random_requests(oracle, 41, 300, 100)
    with V(lib, 0, 0) as v, ThreadPoolExecutor(8) as pool:
        def run(r):
            strict, digest, pks, sigs = r
            if strict:
                ok = v.strict(digest, pks[0], sigs[0])
                return ok, np.array([ok])
            return v.batch(digest, pks, sigs)
        got = list(pool.map(run, reqs))
        st = v.stats()
    assert st["requests"] == 300 and st["bypassed_requests"] == 0, st
    n_bad = 0
    for (strict, digest, pks, sigs), (ok, valid) in zip(reqs, got):
        n = pks.shape[0]
        tiled = np.tile(digest, (n, 1))
        if strict:
            exp = oracle.strict_many(tiled, pks, sigs)
            rc = lib.nwc_verify_strict(_p(digest), _p(pks), _p(sigs))
            assert rc in (0, 1) and (rc == 0) == ok
        else:
            exp = oracle.leaf_many(tiled, pks, sigs)
            bm = np.zeros((n + 7) // 8, np.uint8)
            rc = lib.nwc_verify_batch(_p(digest), _p(pks), _p(sigs), n, _p(bm))
            assert rc in (0, 1) and (rc == 0) == ok
            assert (~np.unpackbits(bm, bitorder="little")[:n].astype(bool) == valid).all()
        assert (valid == exp).all() and ok == bool(exp.all())
        n_bad += not ok
    assert 30 < n_bad < 100, n_bad


def test_lifecycle(lib, oracle):
    from narwhal_amd import _lib
    digest, pks, sigs = _cert(oracle, 51, 1500)
    sigs[[7, 1499], 3] ^= 2
    exp = oracle.leaf_many(np.tile(digest, (1500, 1)), pks, sigs)
    with V(lib, 0, 0) as v:
        ok, valid = v.batch(digest, pks, sigs)   # more than 1,024 votes: handed to nwc_verify_batch
        assert not ok and (valid == exp).all() and list(np.nonzero(~valid)[0]) == [7, 1499]
        st = v.stats()
        assert st["bypassed_requests"] == 1 and st["groups"] == 0 and st["requests"] == 0, st
        assert lib.nwc_verifier_verify_batch(v.h, _p(digest), None, None, 0, None) == 0   # n == 0: Ok at once
        assert v.stats()["requests"] == 0
    small = _cert(oracle, 52, 3)
    mem0 = _lib.memory_info()
    with V(lib, 0, 0) as v1, V(lib, 4, 100) as v2:   # destroyed and created again; two at once on one device
        mem1 = _lib.memory_info()
        for k in ("tables", "committee", "auto_cache", "scratch", "digesters"):
            assert mem1[k] == mem0[k], (k, mem0, mem1)   # group buffers are host memory
        assert v1.batch(*small)[0] and v2.batch(*small)[0]
        assert v1.strict(small[0], small[1][0], small[2][0])
        assert v1.stats()["groups"] == 2 and v2.stats()["groups"] == 1
