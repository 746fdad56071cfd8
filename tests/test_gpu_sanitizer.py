"""GPU tests of nwc_sanitizer (include/nwc.h): concurrent one-message sanitize calls packed into
groups that one set of launches decides (k_parse_group, k_verify_msg_group, k_finalize_group),
every message under its own gc_round and vote target.

Codes, digests and kinds are always compared with tests/golden/messages.json or the CPU restatement
(oracle/messages_ref.py with the C restatement of dalek for signatures), never with the library
alone.  Groups are made deterministic by max_messages: a sanitizer created with (T, seconds)
launches exactly when its T-th message has arrived, and nwc_sanitizer_stats counts a message the
moment it joins a group, so a test can order arrivals -- and with them the slots -- without sleeping."""
import ctypes
import json
import os
import struct
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.test_gpu_messages import _CSig, _install, _random_batch, _sanitize

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "oracle"))

STATS = ("groups", "messages", "bytes", "equations", "redone_messages", "bypassed_messages", "max_messages_in_group",
         "reserved")
LONG_WAIT_US = 5_000_000
NOT_INIT = -3
# the HBM a sanitizer of the default capacity holds (README "Footprint": msg_plan.h san_scratch(256, 1 MiB))
DEFAULT_SCRATCH_BYTES = 2_683_904


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    return _lib.load()


class S:
    """A sanitizer handle; destroyed on exit."""

    def __init__(self, lib, max_messages, max_wait_us):
        self.lib = lib
        self.h = lib.nwc_sanitizer_create(max_messages, max_wait_us)
        assert self.h, lib.nwc_last_error()

    def raw(self, msg, gc_round=0, target=None):
        """(return value, digest, kind)"""
        from narwhal_amd import _lib
        tb = None if target is None else target[0] + struct.pack("<Q", target[1]) + target[2]
        dig, kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
        rc = self.lib.nwc_sanitizer_sanitize(self.h, _lib.buf(msg) if msg else None, len(msg), gc_round,
                                             _lib.buf(tb) if tb else None, dig, kind)
        return rc, dig.raw, kind.raw[0]

    def __call__(self, msg, gc_round=0, target=None):
        rc, dig, kind = self.raw(msg, gc_round, target)
        assert rc >= 0, (rc, self.lib.nwc_last_error())
        return rc, dig, kind

    def stats(self):
        out = (ctypes.c_uint64 * 8)()
        assert self.lib.nwc_sanitizer_stats(self.h, out) == 0
        return dict(zip(STATS, (int(x) for x in out)))

    def wait_messages(self, k):
        while self.stats()["messages"] < k:   # the k-th message has joined its group
            pass

    def close(self):
        if self.h:
            h, self.h = self.h, None
            assert self.lib.nwc_sanitizer_destroy(h) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _one_group(lib, jobs):
    """The jobs (argument tuples of S.__call__) in ONE group, job k in slot k: a sanitizer that
    launches at the len(jobs)-th message, each job started once the previous one has joined."""
    with S(lib, len(jobs), LONG_WAIT_US) as s, ThreadPoolExecutor(len(jobs)) as pool:
        futs = []
        for k, job in enumerate(jobs):
            futs.append(pool.submit(s, *job))
            s.wait_messages(k + 1)
        got = [f.result(timeout=60) for f in futs]
        return got, s.stats()


def _check(got, exp, what):
    """got: (code, digest, kind); exp: mr.sanitize's (code, kind, digest)"""
    code, kind, dig = exp
    assert got[0] == code, (what, got[0], code)
    if kind in (0, 1, 2):
        assert got[1] == dig, what
        assert got[2] == kind, what


def test_golden_messages_each_its_own_call(lib):
    g = json.load(open(os.path.join(GOLDEN, "messages.json")))
    c = g["committee"]
    _install(lib, [bytes.fromhex(k) for k in c["keys"]], c["stakes"], c["workers"])
    cases = g["cases"]
    got = [None] * len(cases)
    try:
        with S(lib, 8, 2000) as s:
            def run(t):
                for i in range(t, len(cases), 8):   # dealt round-robin: a group mixes gc_rounds and targets
                    tj = cases[i]["target"]
                    target = None if tj is None else (bytes.fromhex(tj[0]), tj[1], bytes.fromhex(tj[2]))
                    got[i] = s(bytes.fromhex(cases[i]["msg"]), cases[i]["gc_round"], target)
            threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
            for t in threads:
                t.start()
            for t in threads:
                t.join(timeout=120)
            st = s.stats()
    finally:
        lib.nwc_set_committee(None, 0)
    for case, r in zip(cases, got):
        assert r is not None and r[0] == case["code"], (case["name"], r, case["code_name"])
        if case["kind"] >= 0 and case["kind"] != 3:
            assert r[1].hex() == case["digest"], case["name"]
            assert r[2] == case["kind"], case["name"]
    assert st["messages"] == len(cases) and st["bypassed_messages"] == 0 and st["redone_messages"] == 0, st
    assert st["groups"] < st["messages"] and st["max_messages_in_group"] > 1, st


class _World:
    """A committee of n single-stake authorities signed for by the C oracle, and message builders."""

    def __init__(self, oracle, n, seed):
        import messages_ref as mr
        self.mr, self.o, self.n = mr, oracle, n
        self.rng = np.random.default_rng(seed)
        self.seeds = [bytes(self.rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(n)]
        self.pks = [oracle.public_key(s) for s in self.seeds]
        self.committee = mr.RefCommittee({pk: (1, [0]) for pk in self.pks})
        self.sig = _CSig(oracle)

    def install(self, lib):
        _install(lib, self.pks, [1] * self.n, [[0]] * self.n)

    def rand32(self):
        return bytes(self.rng.integers(0, 256, 32, dtype=np.uint8))

    def header(self, k, rnd, nparents):
        parents = [self.rand32() for _ in range(nparents)]
        hid = self.mr.header_id(self.pks[k], rnd, [], parents)
        return self.mr.enc_header(self.pks[k], rnd, [], parents, hid, self.o.sign(self.seeds[k], hid)), hid

    def certificate(self, k, rnd, voters, nparents=2, bad_vote=None, unpadded_vote=None):
        import base64
        hdr, hid = self.header(k, rnd, nparents)
        cd = self.mr.digest72(hid, rnd, self.pks[k])
        votes = [(self.pks[v], self.o.sign(self.seeds[v], cd)) for v in voters]
        if bad_vote is not None:
            key, s = votes[bad_vote]
            votes[bad_vote] = (key, s[:40] + bytes([s[40] ^ 1]) + s[41:])
        texts = None
        if unpadded_vote is not None:
            texts = [None] * len(votes)
            texts[unpadded_vote] = base64.b64encode(votes[unpadded_vote][0])[:43]   # the voff path
        return self.mr.msg_certificate(hdr, votes, key_texts=texts)

    def vote(self, k, hid, rnd, origin, bad=False):
        s = self.o.sign(self.seeds[k], self.mr.digest72(hid, rnd, origin))
        if bad:
            s = s[:10] + bytes([s[10] ^ 1]) + s[11:]
        return self.mr.msg_vote(hid, rnd, origin, self.pks[k], s)

    def expect(self, msg, gc_round=0, target=None):
        return self.mr.sanitize(msg, self.committee, self.sig, gc_round, target)


def test_per_message_parameters_in_one_group(lib, oracle):
    w = _World(oracle, 4, 5)
    w.install(lib)
    try:
        hid, origin = w.rand32(), w.pks[1]
        vote = w.vote(2, hid, 7, origin)
        hdr = w.mr.msg_header(w.header(0, 5, 3)[0])
        jobs = [(vote, 0, (hid, 7, origin)), (vote, 0, (w.rand32(), 7, origin)), (hdr, 0, None), (hdr, 6, None)]
        exp = [w.expect(*j) for j in jobs]
        assert [e[0] for e in exp] == [0, 9, 0, 7]   # Ok, UnexpectedVote, Ok, TooOld
        # all four behind a barrier: the group closes exactly when the fourth message arrives
        with S(lib, 4, LONG_WAIT_US) as s:
            barrier = threading.Barrier(4)
            got = [None] * 4

            def run(k):
                barrier.wait()
                got[k] = s(*jobs[k])
            threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
            for t in threads:
                t.start()
            for t in threads:
                t.join(timeout=60)
            st = s.stats()
        assert st["groups"] == 1 and st["max_messages_in_group"] == 4 and st["redone_messages"] == 0, st
        for k in range(4):
            _check(got[k], exp[k], k)
    finally:
        lib.nwc_set_committee(None, 0)


@pytest.fixture(scope="module")
def shapes(oracle):
    """A committee of 66 single-stake authorities (quorum 45) and the messages at which the group
    kernels can go wrong, with the restatement's answers (computed once)."""
    w = _World(oracle, 66, 66)
    assert w.committee.quorum_threshold() == 45
    everyone = list(range(66))
    hdr0 = w.mr.msg_header(w.header(3, 4, 0)[0])
    hdr66 = w.mr.msg_header(w.header(4, 4, 66)[0])
    hid = w.rand32()
    m = {
        "garbage": bytes(w.rng.integers(0, 256, 41, dtype=np.uint8)),        # 41 bytes: the next range starts past a gap
        "header-0-parents": hdr0,
        "cert-45": w.certificate(5, 3, everyone[:45]),                         # the plain quorum case
        "vote": w.vote(7, hid, 9, w.pks[8]),
        "five-bytes": b"\x02\x00\x00\x00\x07",
        "header-66-parents": hdr66,
        "cert-65-bad-64": w.certificate(6, 3, everyone[:65], bad_vote=64, unpadded_vote=17),   # odd length, voff path
        "vote-bad-sig": w.vote(9, hid, 9, w.pks[8], bad=True),
        "cert-64": w.certificate(10, 3, everyone[2:66]),                       # exactly one lane stride
        "cert-66": w.certificate(11, 3, everyone, nparents=66),                # the largest vote list the committee allows
        "cert-0": w.certificate(12, 3, []),                                    # RequiresQuorum
        "cert-reuse": w.certificate(13, 3, everyone[:30] + [4] + everyone[30:50]),   # AuthorityReuse
    }
    exp = {k: w.expect(v) for k, v in m.items()}
    assert exp["cert-45"][0] == 0 and exp["cert-64"][0] == 0 and exp["cert-66"][0] == 0
    assert exp["cert-65-bad-64"][0] == 1 and exp["vote-bad-sig"][0] == 1 and exp["cert-0"][0] == 6 and exp["cert-reuse"][0] == 5
    assert exp["garbage"][0] in (8, 10, 11) and exp["five-bytes"][0] == 8 and exp["header-66-parents"][0] == 0
    assert len(m["cert-65-bad-64"]) % 4 != 0 and len(m["garbage"]) % 4 != 0
    return w, m, exp


NINE = ["garbage", "header-0-parents", "cert-45", "vote", "five-bytes", "header-66-parents", "cert-65-bad-64",
        "vote-bad-sig", "cert-64"]


@pytest.mark.parametrize("names", [["cert-66"], ["cert-0", "cert-reuse"], NINE], ids=["1", "2", "9"])
def test_shapes_where_the_kernels_can_go_wrong(lib, shapes, names):
    w, m, exp = shapes
    w.install(lib)
    try:
        got, st = _one_group(lib, [(m[k],) for k in names])
        assert st["groups"] == 1 and st["max_messages_in_group"] == len(names), st
        assert st["redone_messages"] == 0 and st["bypassed_messages"] == 0, st
        for k, r in zip(names, got):
            _check(r, exp[k], k)
        if names is NINE:
            # header, 45 + 1, vote, header, 65 + 1, vote, 64 + 1: what a verdict could depend on, no more
            assert st["equations"] == 1 + 46 + 1 + 1 + 66 + 1 + 65, st
    finally:
        lib.nwc_set_committee(None, 0)


def test_redo_marks_every_third_slot(lib, shapes):
    from narwhal_amd import _lib
    w, m, exp = shapes
    names = NINE + ["cert-66", "cert-0", "cert-reuse"]
    w.install(lib)
    try:
        _lib.diag_set("sanitizer_redo_every", 3)
        got, st = _one_group(lib, [(m[k],) for k in names])
    finally:
        _lib.diag_set("sanitizer_redo_every", 0)
        lib.nwc_set_committee(None, 0)
    assert st["groups"] == 1 and st["max_messages_in_group"] == 12, st
    assert st["redone_messages"] == 4, st   # slots 0, 3, 6 and 9
    for k, r in zip(names, got):
        _check(r, exp[k], k)


def test_random_traffic_vs_oracle_and_the_batch_entry(lib, oracle):
    import messages_ref as mr
    rng = np.random.default_rng(4242)
    committee, pks, stakes, workers, msgs = _random_batch(oracle, rng, N=66, ncert=24, nhdr=12, nvote=12)
    _install(lib, pks, stakes, workers)
    sig = _CSig(oracle)
    try:
        with S(lib, 0, 0) as s, ThreadPoolExecutor(8) as pool:
            got = list(pool.map(lambda b: s(b, 10), msgs))
            st = s.stats()
        codes, dig, kinds = _sanitize(lib, msgs, 10)   # the parent's route, one call
    finally:
        lib.nwc_set_committee(None, 0)
    assert st["messages"] == len(msgs) and st["bypassed_messages"] == 0 and st["redone_messages"] == 0, st
    for i, b in enumerate(msgs):
        exp = mr.sanitize(b, committee, sig, 10)
        _check(got[i], exp, i)
        assert got[i][0] == codes[i], i
        if exp[1] in (0, 1, 2):
            assert got[i][1] == dig[i].tobytes() and got[i][2] == kinds[i], i


def _helper(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sanitizer_helper.py"), mode, ROOT],
                       env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bypass_of_a_message_larger_than_a_group():
    out = _helper("bypass", {"NWC_SANITIZER_GROUP_BYTES": "4096"})
    assert out["cert_len"] > 8192 and out["cert_ok"] and out["vote_ok"], out
    assert out["after_cert"]["bypassed_messages"] == 1 and out["after_cert"]["messages"] == 0, out
    assert out["after_vote"]["bypassed_messages"] == 1 and out["after_vote"]["messages"] == 1 and out["after_vote"]["groups"] == 1, out


def test_bypass_while_the_cache_is_not_the_configured_committee(lib, shapes):
    """After nwc_set_committee the cache is no longer nwc_set_committee_config's: every message is
    handed to nwc_sanitize_messages and answers as it does -- which, the stake tables having gone
    with the configured committee, is NWC_ERR_NOT_INIT until the committee is configured again."""
    from narwhal_amd import _lib
    w, m, exp = shapes
    w.install(lib)
    try:
        with S(lib, 0, 0) as s:
            _check(s(m["vote"]), exp["vote"], "grouped")
            assert s.stats()["bypassed_messages"] == 0
            other = _World(w.o, 4, 99)
            _lib.check(lib.nwc_set_committee(_lib.buf(b"".join(other.pks)), 4))
            codes = np.zeros(1, np.int32)
            offs = np.array([0, len(m["vote"])], np.uint64)
            parent = lib.nwc_sanitize_messages(_lib.buf(m["vote"]), _lib.buf(offs), 1, 0, None, _lib.buf(codes), None, None)
            for name in ("vote", "cert-45"):
                assert s.raw(m[name])[0] == parent == NOT_INIT
            st = s.stats()
            assert st["bypassed_messages"] == 2 and st["messages"] == 1, st
            w.install(lib)   # configured again: grouped again, and right
            _check(s(m["cert-45"]), exp["cert-45"], "configured again")
            assert s.stats()["messages"] == 2
    finally:
        lib.nwc_set_committee(None, 0)


def test_lifecycle_and_memory(lib, shapes):
    from narwhal_amd import _lib
    w, m, exp = shapes
    _lib.check(lib.nwc_set_committee(None, 0))
    assert lib.nwc_sanitizer_create(0, 0) is None   # no configured committee
    assert lib.nwc_last_error_code() == NOT_INIT and b"nwc_set_committee_config" in lib.nwc_last_error()
    w.install(lib)
    try:
        _sanitize(lib, [m["vote"]])   # (the batch entry's own buffers are allocated before the walk)
        mem0 = _lib.memory_info()
        with S(lib, 0, 0) as s1:
            mem1 = _lib.memory_info()
            assert mem1["scratch"] - mem0["scratch"] == DEFAULT_SCRATCH_BYTES, (mem0, mem1)
            with S(lib, 64, LONG_WAIT_US) as s2:   # two at once on one device
                assert _lib.memory_info()["scratch"] > mem1["scratch"]
                _check(s1(m["cert-45"]), exp["cert-45"], "s1")
                _lib.check(lib.nwc_trim())         # a live sanitizer keeps its scratch and goes on working
                assert _lib.memory_info()["scratch"] >= 2 * DEFAULT_SCRATCH_BYTES - (1 << 20)
                _check(s1(m["cert-65-bad-64"]), exp["cert-65-bad-64"], "s1 after trim")
                # destroy with four callers inside: each loops over a few quick calls on s1, then
                # blocks in s2's group, which waits for company; destroy launches that group, and
                # every call returns a right answer (no call may START after destroy, nwc.h)
                names = ["vote", "cert-64", "header-0-parents", "vote-bad-sig"]

                def caller(k):
                    for _ in range(3):
                        _check(s1(m[names[k]]), exp[names[k]], "loop")
                    return s2.raw(m[names[k]])
                with ThreadPoolExecutor(4) as pool:
                    futs = [pool.submit(caller, k) for k in range(4)]
                    s2.wait_messages(4)
                    s2.close()
                    for k, f in enumerate(futs):
                        rc, dig, kind = f.result(timeout=60)
                        assert rc == NOT_INIT or rc >= 0
                        if rc >= 0:
                            _check((rc, dig, kind), exp[names[k]], "destroyed under " + names[k])
        _lib.check(lib.nwc_trim())
        mem2 = _lib.memory_info()
        _sanitize(lib, [m["vote"]])
        with S(lib, 0, 0):
            pass
        _lib.check(lib.nwc_trim())
        assert _lib.memory_info()["scratch"] == mem2["scratch"], (mem2, _lib.memory_info())   # destroy gave it all back
    finally:
        lib.nwc_set_committee(None, 0)


def test_shutdown_retires_a_live_sanitizer():
    out = _helper("shutdown")
    assert out["before"] == 0 and out["after_shutdown"] == NOT_INIT and out["after_reinit"] == NOT_INIT, out
    assert out["destroy"] == 0, out
