"""GPU tests of Vote::new on the device (include/nwc.h: nwc_signer_vote, nwc_signer_vote_many,
nwc_dev_vote, nwc_sanitizer_sanitize_vote, nwc_sanitizer_vote_stats; kernels in csrc/vote.h).

Expected signatures are the pure-Python restatement's, oracle/ed25519_ref.py
sign(seed, digest72(id, round, origin)) with digest72 of oracle/messages_ref.py.  Ed25519 signing is
deterministic, so every comparison is byte-exact.  The restatement takes ~0.2 s per signature: the
257 triples of the signer tests and their signatures are recorded in tests/golden/vote_sigs.json
(tools/gen_vote_golden.py, the same restatement), of which a sample is signed again here; the
dozen header votes of the sanitizer tests are signed once per module.  Codes, digests and kinds of
the sanitizer tests are compared with the CPU restatement and with nwc_sanitizer_sanitize on the
message alone."""
import base64
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
from tests.test_gpu_messages import _install, _sanitize
from tests.test_gpu_sanitizer import LONG_WAIT_US, NOT_INIT, S, _check, _World

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ERR_ARG = -2
NS = [1, 3, 64, 65, 257]


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    return _lib.load()


def make_signer(lib, oracle, seed):
    from narwhal_amd import _lib
    h = lib.nwc_signer_create(_lib.buf(seed + oracle.public_key(seed)))
    assert h, lib.nwc_last_error()
    return h


class SV(S):
    """A sanitizer handle with the vote entry."""

    def vote(self, signer, msg, gc_round=0, target=None):
        """(return value, digest, kind, signature, voted)"""
        from narwhal_amd import _lib
        tb = None if target is None else target[0] + struct.pack("<Q", target[1]) + target[2]
        dig, kind, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1), ctypes.create_string_buffer(b"\xEE" * 64, 64)
        voted = ctypes.c_int32(7)
        rc = self.lib.nwc_sanitizer_sanitize_vote(self.h, signer, _lib.buf(msg) if msg else None, len(msg), gc_round,
                                                  _lib.buf(tb) if tb else None, dig, kind, sig, ctypes.byref(voted))
        return rc, dig.raw, kind.raw[0], sig.raw, voted.value

    def vote_stats(self):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert self.lib.nwc_sanitizer_vote_stats(self.h, ctypes.byref(a), ctypes.byref(b)) == 0
        return {"in_flight": int(a.value), "alone": int(b.value)}

    def group(self, signer, jobs):
        """The jobs -- (msg, gc_round, target, ask) -- in ONE group of this sanitizer, job k in slot
        k: each is started once the previous one has joined.  Jobs that do not ask go through
        nwc_sanitizer_sanitize.  Returns (rc, digest, kind, signature, voted) per job."""
        base = self.stats()["messages"]
        with ThreadPoolExecutor(len(jobs)) as pool:
            futs = []
            for k, (msg, gc, target, ask) in enumerate(jobs):
                if ask:
                    futs.append(pool.submit(self.vote, signer, msg, gc, target))
                else:
                    futs.append(pool.submit(lambda *a: self.raw(*a) + (bytes(64), 0), msg, gc, target))
                self.wait_messages(base + k + 1)
            return [f.result(timeout=60) for f in futs]


# ---- 1. the signer entries -------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(oracle):
    import ed25519_ref as ed
    import messages_ref as mr
    g = json.load(open(os.path.join(GOLDEN, "vote_sigs.json")))
    seed = bytes.fromhex(g["seed"])
    cases = [(bytes.fromhex(c["id"]), c["round"], bytes.fromhex(c["origin"]), bytes.fromhex(c["sig"])) for c in g["cases"]]
    assert len(cases) == 257
    # the first rounds are where the two u32 halves can be swapped or dropped; n = 1 and n = 3 see them too
    assert [c[1] for c in cases[:5]] == [1 << 32, (1 << 64) - 1, (1 << 32) - 1, 0, 1]
    # the file is the restatement's: a sample signed again by it, all of it by the C restatement of dalek
    for i in (0, 1, 64, 256):
        assert ed.sign(seed, mr.digest72(*cases[i][:3])) == cases[i][3], i
    assert ed.public_key(seed).hex() == g["public_key"]
    for i, c in enumerate(cases):
        assert oracle.sign(seed, mr.digest72(*c[:3])) == c[3], i
    return seed, cases


def _arrays(cases, n):
    ids = np.frombuffer(b"".join(c[0] for c in cases[:n]), np.uint8).reshape(n, 32).copy()
    rounds = np.array([c[1] for c in cases[:n]], np.uint64)
    origins = np.frombuffer(b"".join(c[2] for c in cases[:n]), np.uint8).reshape(n, 32).copy()
    return ids, rounds, origins


@pytest.mark.parametrize("path", [1, 2], ids=["lane", "wide"])
@pytest.mark.parametrize("n", NS)
def test_signer_entries_against_the_restatement(lib, oracle, golden, n, path):
    import torch
    from narwhal_amd import _lib, device
    seed, cases = golden
    ids, rounds, origins = _arrays(cases, n)
    want = b"".join(c[3] for c in cases[:n])
    signer = make_signer(lib, oracle, seed)
    try:
        _lib.diag_set("sign_path", path)
        out = np.full((n, 64), 0xEE, np.uint8)
        assert lib.nwc_signer_vote_many(signer, _lib.buf(ids), _lib.buf(rounds), _lib.buf(origins), n, _lib.buf(out)) == 0
        assert out.tobytes() == want
        for i in range(min(n, 3)):   # the one-vote entry (round by value)
            one = ctypes.create_string_buffer(64)
            assert lib.nwc_signer_vote(signer, _lib.buf(cases[i][0]), cases[i][1], _lib.buf(cases[i][2]), one) == 0
            assert one.raw == cases[i][3], i
        dev = torch.device("cuda")
        d_out = device.vote(signer, torch.from_numpy(ids).to(dev), torch.from_numpy(rounds.view(np.int64)).to(dev),
                            torch.from_numpy(origins).to(dev))
        torch.cuda.current_stream().synchronize()
        assert d_out.cpu().numpy().tobytes() == want
        # n == 0 is a no-op; a misaligned device buffer is refused
        assert lib.nwc_signer_vote_many(signer, None, None, None, 0, None) == 0
        t = torch.zeros(128, dtype=torch.uint8, device=dev)
        assert lib.nwc_dev_vote(signer, t.data_ptr() + 1, t.data_ptr(), t.data_ptr(), 1, t.data_ptr(), None) == ERR_ARG
    finally:
        _lib.diag_set("sign_path", 0)
        assert lib.nwc_signer_destroy(signer) == 0


def test_votes_round_trip_through_the_batch_entry(lib, oracle, golden):
    """Each signature, wrapped as the Vote message its (id, round, origin) belong to, sanitizes to Ok
    under that vote target with a committee that holds the signer's key."""
    import messages_ref as mr
    from narwhal_amd import _lib
    seed, cases = golden
    pk = oracle.public_key(seed)
    others = [oracle.public_key(bytes([k]) * 32) for k in (1, 2, 3)]
    n = len(cases)
    ids, rounds, origins = _arrays(cases, n)
    signer = make_signer(lib, oracle, seed)
    _install(lib, [pk] + others, [1] * 4, [[0]] * 4)
    try:
        out = np.zeros((n, 64), np.uint8)
        assert lib.nwc_signer_vote_many(signer, _lib.buf(ids), _lib.buf(rounds), _lib.buf(origins), n, _lib.buf(out)) == 0
        for i, (vid, rnd, origin, _) in enumerate(cases):
            msg = mr.msg_vote(vid, rnd, origin, pk, out[i].tobytes())
            codes, dig, kinds = _sanitize(lib, [msg], 0, (vid, rnd, origin))
            assert codes[0] == 0 and kinds[0] == 1 and dig[0].tobytes() == mr.digest72(vid, rnd, origin), i
        # ... and not under another target, nor with one bit of the signature flipped
        vid, rnd, origin, sig = cases[0]
        assert _sanitize(lib, [mr.msg_vote(vid, rnd, origin, pk, sig)], 0, (vid, rnd ^ (1 << 32), origin))[0][0] == 9
        bad = sig[:5] + bytes([sig[5] ^ 1]) + sig[6:]
        assert _sanitize(lib, [mr.msg_vote(vid, rnd, origin, pk, bad)], 0, (vid, rnd, origin))[0][0] == 1
    finally:
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0


# ---- 2-4. votes in the sanitizer's flight ----------------------------------------------------
@pytest.fixture(scope="module")
def world(oracle):
    """A committee of 4, a signer's seed, the messages of the mixed group with the restatement's
    answers, and the restatement's vote signature for every header whose code is Ok (signed once)."""
    import ed25519_ref as ed
    w = _World(oracle, 4, 77)
    mr = w.mr
    seed = w.rand32()
    outsider = w.rand32()

    def header(k, rnd, nparents, npayload=0, text=None, author=None, seed_=None):
        author = w.pks[k] if author is None else author
        parents = [w.rand32() for _ in range(nparents)]
        payload = [(w.rand32(), 0) for _ in range(npayload)]
        hid = mr.header_id(author, rnd, payload, parents)
        sig = w.o.sign(w.seeds[k] if seed_ is None else seed_, hid)
        return [author, rnd, payload, parents, hid, sig], text

    def wire(h, text=None):
        return mr.msg_header(mr.enc_header(*h, author_text=text))

    hs = {
        "header-a": header(0, 5, 3),
        "header-b": header(1, 6, 2),
        "header-round-2^32": header(2, (1 << 32) + 5, 1),
        "header-round-2^64-1": header(3, (1 << 64) - 1, 1),
        "header-empty": header(3, 4, 0, 0),
        "header-67-parents-3-payload": header(0, 7, 67, 3),
        # key texts that base64 0.13 accepts and base64::encode never emits: the round then sits at
        # another offset, and the origin is the first 32 decoded bytes
        "header-unpadded-key": header(1, 8, 2, text=base64.b64encode(w.pks[1])[:43]),
        "header-long-key": header(2, 9, 2, text=base64.b64encode(w.pks[2] + bytes(range(7)))),
        "header-plain-entry": header(1, 11, 4),
    }
    m = {k: wire(h, t) for k, (h, t) in hs.items()}
    assert len(m["header-unpadded-key"]) % 4 != len(m["header-a"]) % 4 and len(m["header-long-key"]) > len(m["header-b"])
    h, _ = header(0, 5, 2)
    m["header-bad-signature"] = wire(h[:5] + [h[5][:7] + bytes([h[5][7] ^ 4]) + h[5][8:]])
    h, _ = header(1, 5, 2)
    m["header-wrong-id"] = wire(h[:4] + [bytes([h[4][0] ^ 1]) + h[4][1:]] + h[5:])
    m["header-too-old"] = wire(header(2, 5, 2)[0])
    m["header-unknown-author"] = wire(header(0, 5, 2, author=oracle.public_key(outsider), seed_=outsider)[0])
    hid = w.rand32()
    m["vote"] = w.vote(2, hid, 9, w.pks[1])
    m["certificate"] = w.certificate(3, 3, [0, 1, 2])
    m["empty"] = b""
    gc = {k: 0 for k in m}
    gc["header-too-old"] = 6
    exp = {k: w.expect(v, gc[k]) for k, v in m.items()}
    want_codes = {"header-bad-signature": 1, "header-wrong-id": 2, "header-too-old": 7, "header-unknown-author": 4, "empty": 8}
    for k in m:
        assert exp[k][0] == want_codes.get(k, 0), (k, exp[k][0])
    votes = {k: ed.sign(seed, mr.digest72(h[4], h[1], h[0])) for k, (h, _) in hs.items()}
    assert len(set(votes.values())) == len(votes)
    return w, seed, m, gc, exp, votes


MIXED = ["header-a", "header-b", "header-round-2^32", "header-round-2^64-1", "header-empty", "header-67-parents-3-payload",
         "header-unpadded-key", "header-long-key", "header-bad-signature", "header-wrong-id", "header-too-old",
         "header-unknown-author", "vote", "certificate", "empty", "header-plain-entry"]
EIGHT = MIXED[:8]


def _check_votes(names, got, exp, votes, asked):
    """voted is 1 exactly for the Ok headers that asked, with the restatement's bytes; every other
    signature is 64 zero bytes.  Returns how many voted."""
    count = 0
    for k, r in zip(names, got):
        _check(r[:3], exp[k], k)
        if k in asked and exp[k][0] == 0 and exp[k][1] == 0:
            assert r[4] == 1 and r[3] == votes[k], k
            count += 1
        else:
            assert r[4] == 0 and r[3] == bytes(64), k
    return count


def test_one_mixed_group(lib, oracle, world):
    w, seed, m, gc, exp, votes = world
    w.install(lib)
    signer = make_signer(lib, oracle, seed)
    try:
        with S(lib, 0, 0) as plain:
            alone = {k: plain(m[k], gc[k]) for k in MIXED}   # nwc_sanitizer_sanitize on each message alone
        asked = set(MIXED) - {"header-plain-entry"}
        with SV(lib, len(MIXED), LONG_WAIT_US) as s:
            before = s.stats()["groups"]
            got = s.group(signer, [(m[k], gc[k], None, k in asked) for k in MIXED])
            st, vs = s.stats(), s.vote_stats()
        assert st["groups"] - before == 1 and st["max_messages_in_group"] == len(MIXED), st
        assert st["redone_messages"] == 0 and st["bypassed_messages"] == 0, st
        for k, r in zip(MIXED, got):
            assert r[:3] == alone[k], k
        voted = _check_votes(MIXED, got, exp, votes, asked)
        assert voted == 8 and vs == {"in_flight": 8, "alone": 0}, (voted, vs)
    finally:
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0


def test_stale_slots_are_not_signed_for(lib, oracle, world):
    """A voting group of 8, then on the same sanitizer -- the same buffer, every member of the first
    group having left -- a group of 8 without signers: its flight signs nothing."""
    from narwhal_amd import _lib
    w, seed, m, gc, exp, votes = world
    w.install(lib)
    signer = make_signer(lib, oracle, seed)
    try:
        with S(lib, 0, 0) as plain:
            alone = {k: plain(m[k], gc[k]) for k in EIGHT}
        mem0 = _lib.memory_info()
        with SV(lib, 8, LONG_WAIT_US) as s:
            mem1 = _lib.memory_info()
            got = s.group(signer, [(m[k], 0, None, True) for k in EIGHT])
            assert _check_votes(EIGHT, got, exp, votes, set(EIGHT)) == 8
            assert s.vote_stats() == {"in_flight": 8, "alone": 0} and s.stats()["groups"] == 1
            got = s.group(signer, [(m[k], 0, None, False) for k in reversed(EIGHT)])
            assert s.vote_stats() == {"in_flight": 8, "alone": 0} and s.stats()["groups"] == 2
            for k, r in zip(reversed(EIGHT), got):
                assert r[:3] == alone[k] and r[4] == 0, k
            # a third group asks again, in other slots than the first: each vote is its own header's
            got = s.group(signer, [(m[k], 0, None, i % 2 == 0) for i, k in enumerate(reversed(EIGHT))])
            asked = set(list(reversed(EIGHT))[0::2])
            assert _check_votes(list(reversed(EIGHT)), got, exp, votes, asked) == 4
            assert s.vote_stats() == {"in_flight": 12, "alone": 0}
            # the sanitizer's HBM scratch does not grow with voting flights
            mem2 = _lib.memory_info()
            assert {k: mem2[k] for k in ("tables", "committee", "auto_cache", "scratch", "digesters")} == \
                   {k: mem1[k] for k in ("tables", "committee", "auto_cache", "scratch", "digesters")}, (mem1, mem2)
        assert mem1["scratch"] > mem0["scratch"]
    finally:
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0   # after the last vote call


def test_redone_messages_get_their_vote_alone(lib, oracle, world):
    from narwhal_amd import _lib
    w, seed, m, gc, exp, votes = world
    names = EIGHT + ["header-bad-signature", "vote", "certificate", "empty"]
    w.install(lib)
    signer = make_signer(lib, oracle, seed)
    try:
        _lib.diag_set("sanitizer_redo_every", 1)
        with SV(lib, len(names), LONG_WAIT_US) as s:
            got = s.group(signer, [(m[k], 0, None, True) for k in names])
            st, vs = s.stats(), s.vote_stats()
    finally:
        _lib.diag_set("sanitizer_redo_every", 0)
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0
    assert st["groups"] == 1 and st["redone_messages"] == len(names), st
    assert _check_votes(names, got, exp, votes, set(names)) == 8
    assert vs == {"in_flight": 0, "alone": 8}, vs


def test_votes_follow_the_batch_entry_while_the_cache_is_not_the_configured_committee(lib, oracle, world):
    """After nwc_set_committee with other keys the grouped kernels' preconditions no longer hold:
    every message is handed to nwc_sanitize_messages and answers as it does, and a vote is made
    exactly when that answer is Ok -- never for a header the batch entry did not accept."""
    from narwhal_amd import _lib
    w, seed, m, gc, exp, votes = world
    w.install(lib)
    signer = make_signer(lib, oracle, seed)
    try:
        with SV(lib, 0, 0) as s:
            other = _World(w.o, 4, 99)
            _lib.check(lib.nwc_set_committee(_lib.buf(b"".join(other.pks)), 4))
            for k in ("header-a", "header-long-key", "header-bad-signature", "vote"):
                codes = np.zeros(1, np.int32)
                offs = np.array([0, len(m[k])], np.uint64)
                parent = lib.nwc_sanitize_messages(_lib.buf(m[k]), _lib.buf(offs), 1, 0, None, _lib.buf(codes), None, None)
                parent = int(codes[0]) if parent >= 0 else parent
                rc, dig, kind, sig, voted = s.vote(signer, m[k])
                assert rc == parent, (k, rc, parent)
                if rc == 0 and exp[k][1] == 0:
                    assert voted == 1 and sig == votes[k], k
                else:
                    assert voted == 0 and sig == bytes(64), k
            assert s.stats()["bypassed_messages"] == 4 and s.stats()["messages"] == 0
            assert s.vote_stats()["in_flight"] == 0
            w.install(lib)   # configured again: grouped again, the vote from the flight
            rc, dig, kind, sig, voted = s.vote(signer, m["header-long-key"])
            assert (rc, voted, sig) == (0, 1, votes["header-long-key"])
            assert s.vote_stats()["in_flight"] == 1
    finally:
        lib.nwc_set_committee(None, 0)
        assert lib.nwc_signer_destroy(signer) == 0


# ---- 4b, 5, 6: in child processes ------------------------------------------------------------
def _helper(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vote_helper.py"), mode, ROOT],
                       env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bypassed_header_still_returns_its_exact_vote():
    out = _helper("bypass", {"NWC_SANITIZER_GROUP_BYTES": "4096"})
    assert out["len"] > 4096 and out["ok"] and out["voted"] == 1 and out["sig_ok"], out
    assert out["stats"]["bypassed_messages"] == 1 and out["stats"]["messages"] == 0, out
    assert out["vote_stats"] == {"in_flight": 0, "alone": 1} and out["destroy"] == 0, out


def test_signer_of_another_device_is_refused():
    out = _helper("wrong_device", {"NWC_VIRTUAL_DEVICES": "2"})
    assert out["devices"] == 2, out
    assert out["rc"] == ERR_ARG and out["code"] == ERR_ARG and out["voted"] == 0 and out["sig_zero"], out
    st = out["stats_after_refusal"]
    assert st["messages"] == 0 and st["groups"] == 0 and st["bypassed_messages"] == 0, out   # nothing was queued or launched
    assert out["same_device"] == [0, 1, True] and out["destroy"] == [0, 0], out


def test_shutdown_with_a_live_sanitizer_and_signer():
    out = _helper("shutdown")
    assert out["before"] == [0, 1], out
    assert out["after_shutdown"] == [NOT_INIT, 0, True] and out["destroy"] == [0, 0], out
