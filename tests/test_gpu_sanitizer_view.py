"""GPU tests of the decoded views from the sanitizer handle's group flight
(nwc_sanitizer_sanitize_view, nwc_sanitizer_view_stats, k_view_group).

Every record is checked field for field against tests/msg_view_model.py -- the independent reference,
which stands on oracle/messages_ref.py `decode` -- and, all 160 bytes with
body_used and the body areas the record names, against nwc_sanitize_messages_view on the same message
alone (tests/sanitizer_view_helper.py: check_answer); that second comparison shows the two routes
agree, no more, since their kernels share message_view.  The committee of 66 and the shapes are those
of tests/test_gpu_sanitizer.py, the builders of unsorted sequences those of
tests/test_gpu_msg_view.py.  Groups are made deterministic as there: a sanitizer created with
(T, seconds) launches exactly when its T-th message has arrived."""
import ctypes
import json
import os
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.msg_view_helper import Model
from tests.sanitizer_view_helper import ERR_ARG, SW, alone, check_answer
from tests.test_gpu_messages import _CSig, _install, _random_batch
from tests.test_gpu_msg_view import _entries, _message, _shuffled
from tests.test_gpu_sanitizer import LONG_WAIT_US, NINE, NOT_INIT, DEFAULT_SCRATCH_BYTES, S, shapes  # noqa: F401  (shapes: a fixture)
from tests.test_gpu_vote import SV, make_signer

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HELPER = os.path.join(ROOT, "tests", "sanitizer_view_helper.py")


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def eleven(shapes):  # noqa: F811
    """The nine shapes between a header of 65 parents shuffled with duplicates and a header of 600
    unsorted payload entries (above the 512 at which canon_entries changes network)."""
    w, m, exp = shapes
    m = dict(m)
    m["hdr-65-shuffled"] = _message(w, [], _shuffled(w, _entries(w, 65)), author=1)
    dig = _entries(w, 600)
    m["hdr-600-unsorted"] = _message(w, [(d, 100 + j) for j, d in enumerate(_shuffled(w, dig))], _entries(w, 3), author=2)
    names = ["hdr-65-shuffled"] + NINE + ["hdr-600-unsorted"]
    return w, m, exp, names, Model(w.pks)


# ---- 1. the golden wire fixtures -------------------------------------------------------------------
def test_golden_fixtures_one_call_each(lib):
    g = json.load(open(os.path.join(GOLDEN, "messages.json")))
    c = g["committee"]
    keys = [bytes.fromhex(k) for k in c["keys"]]
    _install(lib, keys, c["stakes"], c["workers"])
    model = Model(keys)
    try:
        with SW(lib, 0, 0) as s:
            flags = 0
            for case in g["cases"]:
                t = case["target"]
                item = (bytes.fromhex(case["msg"]), case["gc_round"], None if t is None else (bytes.fromhex(t[0]), t[1], bytes.fromhex(t[2])))
                a = s.view(*item)
                assert a.rc == case["code"], (case["name"], a.rc)
                check_answer(lib, model, item, a, case["name"])
                assert int(a.rec[0]) == (0 if case["code"] in (8, 10, 11) else 1), case["name"]
                flags |= int(a.rec[2])
            st, vs = s.stats(), s.view_stats()
        assert flags == 3   # some fixture has its payload, some its parents in the body
        assert st["messages"] == len(g["cases"]) and st["redone_messages"] == 0 and st["bypassed_messages"] == 0, st
        assert vs == {"in_flight": len(g["cases"]), "alone": 0}, vs
    finally:
        lib.nwc_set_committee(None, 0)


# ---- 2. one group of eleven ------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1], ids=["even-slots-ask", "odd-slots-ask"])
def test_one_group_of_eleven(lib, oracle, eleven, parity):
    """Slots ask for a view alternately; the two Ok headers also ask for a vote (with even slots
    asking they are viewers too, with odd slots asking they take the vote entry: view == NULL)."""
    from narwhal_amd import _lib
    w, m, exp, names, model = eleven
    w.install(lib)
    seed = w.rand32()
    signer = make_signer(lib, oracle, seed)
    voters = {"header-0-parents": (3, 4), "header-66-parents": (4, 4)}   # name -> (author, round)
    try:
        with S(lib, 0, 0) as plain:
            lone = {k: plain(m[k]) for k in names}   # nwc_sanitizer_sanitize on each message alone
        with SW(lib, 11, LONG_WAIT_US) as s:
            jobs = [(m[k], 0, None, i % 2 == parity, signer if k in voters else None) for i, k in enumerate(names)]
            got = s.group(jobs)
            st, vs = s.stats(), s.view_stats()
        askers = [k for i, k in enumerate(names) if i % 2 == parity]
        assert st["groups"] == 1 and st["max_messages_in_group"] == 11 and st["redone_messages"] == 0, st
        assert st["bypassed_messages"] == 0, st
        assert vs == {"in_flight": len(askers), "alone": 0}, vs
        for i, (k, a) in enumerate(zip(names, got)):
            assert a.plain() == lone[k], k
            if k in exp:
                assert a.rc == exp[k][0], k
            if k in voters:
                # Vote::new(header, signer's key): what nwc_signer_vote signs for (id, round, origin)
                author, rnd = voters[k]
                want = ctypes.create_string_buffer(64)
                assert lib.nwc_signer_vote(signer, _lib.buf(exp[k][2]), rnd, _lib.buf(w.pks[author]), want) == 0
                assert a.rc == 0 and a.voted == 1 and a.sig == want.raw, k
            if i % 2 == parity:
                check_answer(lib, model, (m[k], 0, None), a, k, signer=signer if k in voters else None)
            else:
                assert (a.rec == 0xEE).all() and (a.body == 0xEE).all() and a.used == 0xEEEE, k
        by = dict(zip(names, got))
        if parity == 0:
            r = by["hdr-65-shuffled"].rec
            assert (int(r[0]), int(r[2])) == (1, 2) and struct.unpack_from("<II", r.tobytes(), 120) == (0, 65)
            r = by["hdr-600-unsorted"].rec
            assert (int(r[0]), int(r[2])) == (1, 1) and struct.unpack_from("<II", r.tobytes(), 120) == (600, 3)
            assert by["hdr-600-unsorted"].used == (36 * 602 + 15) // 16 * 16
        else:
            r = by["cert-65-bad-64"].rec   # the unpadded key string: the parse's voff[] entries
            assert int(r[0]) == 1 and struct.unpack_from("<I", r.tobytes(), 128)[0] == 65
            assert by["garbage"].rec[0] == 0 and by["five-bytes"].rec[0] == 0
    finally:
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0


# ---- 3. stale slots --------------------------------------------------------------------------------
def test_stale_slots_get_no_view(lib, eleven):
    w, m, exp, names, model = eleven
    four = ["hdr-65-shuffled", "cert-45", "vote", "header-66-parents"]
    w.install(lib)
    try:
        with S(lib, 0, 0) as plain:
            lone = {k: plain(m[k]) for k in four}
        with SW(lib, 4, LONG_WAIT_US) as s:
            got = s.group([(m[k], 0, None, True, None) for k in four])
            for k, a in zip(four, got):
                check_answer(lib, model, (m[k], 0, None), a, k)
            assert s.view_stats() == {"in_flight": 4, "alone": 0} and s.stats()["groups"] == 1
            # the second buffer, then the first one again: every member of the first group has left
            for rnd in (2, 3):
                got = s.group([(m[k], 0, None, False, None) for k in reversed(four)])
                for k, a in zip(reversed(four), got):
                    assert a.plain() == lone[k], (rnd, k)
                    assert (a.rec == 0xEE).all() and a.used == 0xEEEE, (rnd, k)
                assert s.view_stats() == {"in_flight": 4, "alone": 0} and s.stats()["groups"] == rnd
            # a fourth group asks again, in other slots than the first: each view is its own message's
            got = s.group([(m[k], 0, None, i % 2 == 0, None) for i, k in enumerate(reversed(four))])
            for i, (k, a) in enumerate(zip(reversed(four), got)):
                assert a.plain() == lone[k], k
                if i % 2 == 0:
                    check_answer(lib, model, (m[k], 0, None), a, k)
            assert s.view_stats() == {"in_flight": 6, "alone": 0} and s.stats()["redone_messages"] == 0
    finally:
        lib.nwc_set_committee(None, 0)


# ---- 4. redo ---------------------------------------------------------------------------------------
def test_redone_messages_get_their_view_alone(lib, eleven):
    from narwhal_amd import _lib
    w, m, exp, names, model = eleven
    twelve = NINE + ["cert-66", "cert-0", "cert-reuse"]
    jobs = [(m[k], 0, None, True, None) for k in twelve]
    w.install(lib)
    try:
        with SW(lib, 12, LONG_WAIT_US) as s:
            flight = s.group(jobs)
            assert s.view_stats() == {"in_flight": 12, "alone": 0} and s.stats()["redone_messages"] == 0
        try:
            _lib.diag_set("sanitizer_redo_every", 3)
            with SW(lib, 12, LONG_WAIT_US) as s:
                got = s.group(jobs)
                st, vs = s.stats(), s.view_stats()
        finally:
            _lib.diag_set("sanitizer_redo_every", 0)
        assert st["groups"] == 1 and st["redone_messages"] == 4, st   # slots 0, 3, 6 and 9
        assert vs == {"in_flight": 8, "alone": 4}, vs
        for k, a, b in zip(twelve, got, flight):
            assert a.rc == exp[k][0], k
            check_answer(lib, model, (m[k], 0, None), a, k)
            check_answer(lib, model, (m[k], 0, None), b, k)
            assert a.plain() == b.plain() and a.rec.tobytes() == b.rec.tobytes() and a.used == b.used, k
    finally:
        lib.nwc_set_committee(None, 0)


# ---- 5, 6c, 9: in child processes ------------------------------------------------------------------
def _child(mode, env=None):
    r = subprocess.run([sys.executable, HELPER, mode, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bypassed_messages_return_their_exact_view():
    out = _child("bypass", {"NWC_SANITIZER_GROUP_BYTES": "4096"})
    assert out["cert_len"] > 8192 and out["cert_ok"], out
    a = out["after_cert"]
    assert (a["bypassed_messages"], a["messages"], a["in_flight"], a["alone"]) == (1, 0, 0, 1), out
    a = out["after_vote"]
    assert (a["bypassed_messages"], a["messages"], a["groups"], a["in_flight"], a["alone"]) == (1, 1, 1, 1, 1), out
    # while the cache is not the configured committee the call answers as nwc_sanitize_messages_view
    u = out["unconfigured"]
    assert u["rc"] == u["parent"] == NOT_INIT and u["record_zero"] and u["parent_record_zero"], out
    assert u["used"] == u["parent_used"] == 0, out
    a = out["after_unconfigured"]
    assert (a["bypassed_messages"], a["messages"], a["in_flight"], a["alone"]) == (2, 1, 1, 1), out
    a = out["after_configured"]
    assert (a["bypassed_messages"], a["messages"], a["in_flight"], a["alone"]) == (2, 2, 2, 1), out


def test_a_sanitizer_holds_the_same_scratch_with_and_without_views():
    out = _child("scratch")
    assert out["at_create"] == DEFAULT_SCRATCH_BYTES, out   # the layout before views existed, to the byte
    assert out["null_view_same"] and out["never_viewed"] == DEFAULT_SCRATCH_BYTES, out
    assert out["after_views"] == DEFAULT_SCRATCH_BYTES and out["view_stats"] == {"in_flight": 1, "alone": 0}, out


def test_shutdown_with_viewers_inside():
    out = _child("shutdown")
    assert len(out["rcs"]) == 4 and all(rc == NOT_INIT or rc >= 0 for rc in out["rcs"]), out
    assert out["right"] == sum(1 for rc in out["rcs"] if rc >= 0), out
    assert out["after_shutdown"] == [NOT_INIT, True, 0] and out["destroy"] == 0, out


# ---- 6. view == NULL is the vote entry -------------------------------------------------------------
def test_null_view_is_the_vote_entry(lib, oracle, eleven):
    w, m, exp, names, model = eleven
    w.install(lib)
    signer = make_signer(lib, oracle, w.rand32())
    try:
        with SV(lib, 0, 0) as v, SW(lib, 0, 0) as s:
            for k in ("header-0-parents", "cert-45", "vote-bad-sig", "garbage", "hdr-65-shuffled"):
                want = v.vote(signer, m[k])
                a = s.view(m[k], signer=signer, view=False)
                assert (a.rc, a.dig, a.kind, a.sig, a.voted) == want, k
                assert (a.rec == 0xEE).all() and (a.body == 0xEE).all() and a.used == 0xEEEE, k   # body arguments untouched
                a = s.view(m[k], view=False)
                assert a.plain() == v.raw(m[k]) and a.voted == 7 and a.sig == b"\xEE" * 64, k
                assert (a.body == 0xEE).all() and a.used == 0xEEEE, k
            assert s.view_stats() == {"in_flight": 0, "alone": 0}
            # a body below the bound: refused before anything is queued
            before = s.stats()
            msg = m["header-66-parents"]
            a = s.view(msg, cap=len(msg) + 63)
            assert a.rc == ERR_ARG and lib.nwc_last_error_code() == ERR_ARG, a.rc
            assert (a.rec == 0).all() and a.used == 0 and (a.body == 0xEE).all()
            assert s.stats() == before and s.view_stats() == {"in_flight": 0, "alone": 0}
            a = s.view(msg, cap=len(msg) + 64)   # the bound itself is enough
            check_answer(lib, model, (msg, 0, None), a, "cap == bound")
    finally:
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0


# ---- 7. random traffic -----------------------------------------------------------------------------
def test_random_traffic_all_asking(lib, oracle):
    import messages_ref as mr
    rng = np.random.default_rng(4242)
    committee, pks, stakes, workers, msgs = _random_batch(oracle, rng, N=66, ncert=24, nhdr=12, nvote=12)
    _install(lib, pks, stakes, workers)
    sig = _CSig(oracle)
    model = Model(pks)
    try:
        with SW(lib, 0, 0) as s, ThreadPoolExecutor(8) as pool:
            got = list(pool.map(lambda b: s.view(b, 10), msgs))
            st, vs = s.stats(), s.view_stats()
        assert st["messages"] == len(msgs) and st["bypassed_messages"] == 0 and st["redone_messages"] == 0, st
        assert vs == {"in_flight": len(msgs), "alone": 0}, vs
        for i, (b, a) in enumerate(zip(msgs, got)):
            e = mr.sanitize(b, committee, sig, 10)
            assert a.rc == e[0], (i, a.rc, e[0])
            check_answer(lib, model, (b, 10, None), a, i)
    finally:
        lib.nwc_set_committee(None, 0)


# ---- 8. the Python mirror --------------------------------------------------------------------------
def test_mirror_sanitizer_sanitize_view(lib):
    """narwhal_amd.messages.Sanitizer.sanitize_view rebuilds the objects whose to_bytes() made the
    wires, and answers as sanitize_vote does."""
    from narwhal_amd.crypto import Digest, PublicKey, SecretKey, Signature, Signer
    from narwhal_amd.messages import Authority, Certificate, Committee, Header, Sanitizer, Vote
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verify.json")))
    keys = [(PublicKey(bytes.fromhex(p)), SecretKey(bytes.fromhex(s) + bytes.fromhex(p)))
            for s, p in zip(g["reference_keys"]["seeds"], g["reference_keys"]["pks"])]
    committee = Committee({pk: Authority(1, [0]) for pk, _ in keys})
    rng = np.random.default_rng(12)
    r32 = lambda: Digest(bytes(rng.integers(0, 256, 32, dtype=np.uint8)))  # noqa: E731
    committee.install()
    try:
        parents = {c.digest() for c in Certificate.genesis(committee)}
        hdr = Header.new(keys[0][0], 1, {r32(): 0, r32(): 0, r32(): 0}, parents, keys[0][1])
        vote = Vote.new(hdr, keys[1][0], keys[1][1])
        outsider = PublicKey(bytes(rng.integers(0, 256, 32, dtype=np.uint8)))
        cert = Certificate(hdr, [(k, Signature.new(Certificate(hdr).digest(), s)) for k, s in keys[1:]] + [(outsider, Signature())])
        ps = sorted(bytes(p) for p in hdr.parents)
        wire = hdr.to_bytes()
        at = wire.index(b"".join(ps))
        byz = wire[:at - 8] + struct.pack("<Q", len(ps) + 1) + b"".join(reversed(ps)) + ps[0] + wire[at + 32 * len(ps):]
        msgs = [hdr.to_bytes(), vote.to_bytes(), cert.to_bytes(), byz, b"\x03\0\0\0", hdr.to_bytes()[:-1]]
        signer = Signer(keys[2][1])
        with Sanitizer(committee=committee) as s:
            got = [s.sanitize_view(b) for b in msgs]
            assert [g_[4] for g_ in got[:4]] == [hdr, vote, cert, hdr]
            assert got[4][4] is None and got[5][4] is None
            assert [g_[:3] for g_ in got] == [s.sanitize(b) for b in msgs]
            assert all(g_[3] is None for g_ in got)
            code, dig, kind, sig, obj = s.sanitize_view(msgs[0], signer=signer)
            assert (code, dig, kind, sig) == s.sanitize_vote(msgs[0], signer) and sig is not None and obj == hdr
            assert s.view_stats() == {"in_flight": 7, "alone": 0}
        signer.close()
    finally:
        lib.nwc_set_committee(None, 0)
