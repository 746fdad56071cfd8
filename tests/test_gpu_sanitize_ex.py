"""GPU tests of the batch entries with per-message Core state and Vote::new (include/nwc.h:
nwc_sanitize_messages_ex, nwc_dev_sanitize_messages_ex; k_parse_messages_own in csrc/messages.h,
k_vote_msgs in csrc/vote.h).

Every comparison is exact.  Codes, digests and kinds are compared with nwc_sanitize_messages called
on each message alone under that message's state (the entry the new ones must agree with) AND with
the CPU restatement (oracle/messages_ref.py sanitize, signatures by the C restatement of dalek).
Vote signatures are compared with nwc_signer_vote(id, round, author) and with the C restatement's
sign(seed, Vote::digest); Ed25519 signing is deterministic.  The wire messages
(tests/sanitize_ex_helper.py fixture) are built once per module with messages_ref's encoders over
four single-stake keys and one key without stake; the signer's key is one of the four."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT
from tests.test_gpu_messages import _sanitize
from tests.sanitize_ex_helper import (EXPECTED_CODES, SIGNER_KEY, VOTE_BATCH, ExWorld, dev_ex, fixture, run_ex, vote_batch)

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ERR_ARG = -2
HELPER = os.path.join(ROOT, "tests", "sanitize_ex_helper.py")


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    return _lib.load()


class Ref:
    """The two references, each computed once per distinct (message, gc_round, target)."""

    def __init__(self, lib, w):
        self.lib, self.w, self.alone, self.cpu = lib, w, {}, {}

    def of(self, item):
        if item not in self.alone:
            c, d, k = _sanitize(self.lib, [item[0]], item[1], item[2])
            self.alone[item] = (int(c[0]), bytes(d[0]), int(k[0]))
            self.cpu[item] = self.w.expect(*item)
        return self.alone[item], self.cpu[item]


@pytest.fixture(scope="module")
def world(lib, oracle):
    from narwhal_amd import _lib
    w = ExWorld(oracle)
    w.install(lib)
    f = fixture(w)
    seed = w.seeds[SIGNER_KEY]
    signer = lib.nwc_signer_create(_lib.buf(seed + w.pks[SIGNER_KEY]))
    assert signer, lib.nwc_last_error()
    ref = Ref(lib, w)
    # the fixture is what its names say, by the CPU restatement
    for name, item in f.items():
        assert ref.of(item)[1][0] == EXPECTED_CODES[name], (name, ref.of(item)[1][0])
    yield w, f, signer, ref
    assert lib.nwc_signer_destroy(signer) == 0
    lib.nwc_set_committee(None, 0)


def check_verdicts(got, items, ref, what):
    codes, dig, kinds = got[:3]
    for i, item in enumerate(items):
        alone, cpu = ref.of(item)
        assert (int(codes[i]), bytes(dig[i]), int(kinds[i])) == alone, (what, i, int(codes[i]), alone[0])
        code, kind, d = cpu
        assert int(codes[i]) == code, (what, i, int(codes[i]), code)
        if kind in (0, 1, 2):
            assert bytes(dig[i]) == d and int(kinds[i]) == kind, (what, i)


def expected_vote(lib, w, signer, item, cpu):
    """(voted, signature) by nwc_signer_vote over the restatement's decoding of the header, checked
    against the C restatement's signature of Vote::digest."""
    from narwhal_amd import _lib
    code, kind, dig = cpu
    if not (code == 0 and kind == 0):
        return 0, bytes(64)
    k, fields = w.mr.decode(item[0])
    assert k == 0 and w.mr.header_digest(fields) == dig == fields["id"]
    sig = ctypes.create_string_buffer(64)
    _lib.check(lib.nwc_signer_vote(signer, _lib.buf(dig), fields["round"], _lib.buf(fields["author"]), sig))
    assert sig.raw == w.o.sign(w.seeds[SIGNER_KEY], w.mr.digest72(dig, fields["round"], fields["author"]))
    return 1, sig.raw


def check_votes(lib, w, signer, got, items, ref, what):
    sigs, voted = got[3], got[4]
    for i, item in enumerate(items):
        v, s = expected_vote(lib, w, signer, item, ref.of(item)[1])
        assert int(voted[i]) == v, (what, i, int(voted[i]), v)
        assert bytes(sigs[i]) == s, (what, i)


def mixed(f, m):
    """m messages that mix headers, votes, certificates, a CertificatesRequest, a truncated and an
    empty message, each under its own (gc_round, target)."""
    names = ["cert-ok", "hdr-ok", "vote-ok", "request", "hdr-too-old", "truncated", "vote-stale-target", "empty",
             "cert-too-old", "hdr-at-gc", "vote-old", "hdr-long-key", "cert-bad-vote", "vote-no-target", "hdr-bad-id",
             "hdr-no-stake", "hdr-bad-sig", "hdr-ok-last"]
    return [f[names[i % len(names)]] for i in range(m)]


# ---- 1. equivalence ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 65])
def test_each_message_as_alone_under_its_own_state(lib, world, m):
    w, f, signer, ref = world
    items = mixed(f, m)
    check_verdicts(run_ex(lib, items), items, ref, "m=%d" % m)
    # with a signer the verdicts are the same, and a caller that takes no digests still gets its votes
    got = run_ex(lib, items, signer)
    check_verdicts(got, items, ref, "m=%d signer" % m)
    check_votes(lib, w, signer, got, items, ref, "m=%d" % m)
    nod = run_ex(lib, items, signer, digests=False)
    assert (nod[0] == got[0]).all() and (nod[3] == got[3]).all() and (nod[4] == got[4]).all()
    assert (nod[1] == 0xEE).all()
    # one of the two arrays alone: the call-wide value holds for the other
    hid, rnd, origin = f["vote-ok"][2]
    gc_only = [(it[0], it[1], (hid, rnd, origin)) for it in items]
    check_verdicts(run_ex(lib, gc_only, own_state="gc", target=(hid, rnd, origin)), gc_only, ref, "m=%d gc_rounds alone" % m)
    tg_only = [(it[0], 4, it[2]) for it in items]
    check_verdicts(run_ex(lib, tg_only, own_state="targets", gc_round=4), tg_only, ref, "m=%d targets alone" % m)


# ---- 2. the state is per message ----------------------------------------------------------------
def test_state_is_per_message_inside_a_call_and_across_the_64_boundary(lib, world):
    w, f, signer, ref = world
    hdr = (f["hdr-at-gc"], f["hdr-too-old"])          # one header, gc_round on either side of its round
    vote = (f["vote-ok"], f["vote-stale-target"])     # one vote, a matching and a stale target
    assert hdr[0][0] == hdr[1][0] and vote[0][0] == vote[1][0]
    fill = [f["cert-ok"], f["hdr-ok"], f["vote-no-target"]]
    for first, second in ((hdr, vote), (vote, hdr)):
        items = [fill[i % 3] for i in range(70)]
        items[10], items[11] = first          # inside one verdict word
        items[63], items[64] = second         # adjacent across the 64-message boundary
        got = run_ex(lib, items, signer)
        check_verdicts(got, items, ref, "pairs")
        check_votes(lib, w, signer, got, items, ref, "pairs")
        pair = {id(hdr): [0, 7], id(vote): [0, 9]}   # Ok, TooOld; Ok, UnexpectedVote
        assert [int(got[0][10]), int(got[0][11])] == pair[id(first)]
        assert [int(got[0][63]), int(got[0][64])] == pair[id(second)]


# ---- 3. votes -----------------------------------------------------------------------------------
def test_votes_for_ok_headers_only(lib, world):
    w, f, signer, ref = world
    items = vote_batch(f)
    assert VOTE_BATCH[-1] == "hdr-ok-last"
    got = run_ex(lib, items, signer)
    check_verdicts(got, items, ref, "votes")
    check_votes(lib, w, signer, got, items, ref, "votes")
    codes, _, kinds, sigs, voted = got
    want = [1 if n in ("hdr-ok", "hdr-long-key", "hdr-ok-last") else 0 for n in VOTE_BATCH]
    assert [int(v) for v in voted] == want
    for i, n in enumerate(VOTE_BATCH):
        if kinds[i] != 0 or codes[i] != 0:
            assert voted[i] == 0 and not sigs[i].any(), n
    # the vote is over the parsed key, not its text: the 48-symbol author is the committee's fourth key
    k, fields = w.mr.decode(f["hdr-long-key"][0])
    assert fields["author"] == w.pks[3]


def test_null_state_and_no_signer_is_the_plain_entry(lib, world):
    w, f, signer, ref = world
    items = vote_batch(f) + mixed(f, 60)
    hid, rnd, origin = f["vote-ok"][2]
    for gc, target in ((0, None), (6, (hid, rnd, origin)), (3, (w.rand32(), rnd, origin))):
        plain = _sanitize(lib, [it[0] for it in items], gc, target)
        got = run_ex(lib, items, None, own_state=False, gc_round=gc, target=target)
        for a, b in zip(got[:3], plain):
            assert a.tobytes() == b.tobytes()
        assert (got[3] == 0xEE).all() and (got[4] == 0xEE).all()   # untouched without a signer


# ---- 4. staged and chunked ------------------------------------------------------------------------
def _child(mode, env):
    r = subprocess.run([sys.executable, HELPER, mode, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_staged_and_chunked_call():
    got = _child("chunked", {"NWC_MSG_CHUNK": "1048576"})
    print({k: v for k, v in got.items() if k != "cuts"}, got["cuts"])
    cuts = got["cuts"]
    assert (4 << 20) <= got["total"] < (4 << 20) + 65536 and got["calls"] >= 4
    assert len(cuts) >= 4 and cuts[0] == 0 and cuts[-1] == got["m"] and all(c % 64 == 0 for c in cuts[1:-1]), cuts
    assert got["same"] == [True] * 5, got["same"]
    assert got["same_twice"] == [True] * 5, got["same_twice"]
    assert got["same_without_signer"] == [True] * 3
    # the edges' stale state changed verdicts there and nowhere else
    assert got["edges"] == 2 * (len(cuts) - 1) and got["edge_codes_differ"] >= len(cuts) - 1, got
    assert got["neighbours_unchanged"]
    assert all(v > 0 for v in got["voted_per_chunk"]), got["voted_per_chunk"]   # Ok headers in every chunk
    assert got["voted_is_ok_header"] and got["unvoted_sigs_zero"] and got["destroy"] == 0


# ---- 5. the device entry ------------------------------------------------------------------------
def test_device_entry_on_a_side_stream(lib, world):
    import torch
    w, f, signer, ref = world
    items = vote_batch(f)
    host = run_ex(lib, items, signer)
    rc, got = dev_ex(lib, items, signer, torch.cuda.Stream())
    assert rc == 0, lib.nwc_last_error()
    for a, b in zip(got, host):
        assert a.tobytes() == b.tobytes()
    check_votes(lib, w, signer, got, items, ref, "device")
    # without a signer: the same verdicts, the vote outputs untouched (none were passed)
    rc, plain = dev_ex(lib, items, None, torch.cuda.Stream())
    assert rc == 0, lib.nwc_last_error()
    for a, b in zip(plain[:3], host[:3]):
        assert a.tobytes() == b.tobytes()
    assert (plain[3] == 0xEE).all() and (plain[4] == 0xEE).all()


# ---- 6. a signer of another device ----------------------------------------------------------------
def test_signer_of_another_device(lib, world):
    w, f, signer, ref = world
    got = _child("wrong_device", {"NWC_VIRTUAL_DEVICES": "2"})
    assert got["devices"] == 2
    assert got["dev_rc"] == ERR_ARG and got["dev_code"] == ERR_ARG and got["dev_votes_zero"], got
    assert got["dev_rc_same_device"] == 0 and got["dev_matches"] == [True] * 5, got
    assert got["host_matches"] == [True] * 5, got
    # the host call with the signer of context 1 gave what this process's signer gives (test 3's batch)
    here = run_ex(lib, vote_batch(f), signer)
    assert got["codes"] == [int(c) for c in here[0]] and got["voted"] == [int(v) for v in here[4]]
    assert got["sigs"] == bytes(here[3]).hex()
    # the call without a signer, split over both contexts: every message still under its own state
    assert got["sharded_m"] >= 4096 and got["sharded_codes_ok"] and got["sharded_kinds_ok"], got
    assert got["destroy"] == [0, 0]


# ---- 7. memory ------------------------------------------------------------------------------------
def test_no_signing_table_without_a_signer():
    got = _child("memory", {})
    assert got["tables_start"] == 0 and got["sign_table_start"] == 0, got
    assert got["codes"] == [0, 0, 0, 7, 8] and got["codes_plain"] == [0, 0, 0, 0, 8], got
    assert got["sign_table_after_ex"] == 0, got            # the call built the verification tables only
    assert got["tables_after_ex"] > (2 << 30), got
    assert got["sign_table_with_signer"], got
    assert 0 < got["tables_with_signer"] - got["tables_after_ex"] < (1 << 20), got   # the signer's 60 KB
    assert got["voted"] == [1, 0, 0, 0, 0] and got["destroy"] == 0, got


# ---- the Python mirror ----------------------------------------------------------------------------
def test_mirror_sanitize_many_ex(lib):
    """narwhal_amd.messages.sanitize_many_ex: a batch drained across a round boundary -- votes for the
    old and the new header, each judged under the state recorded with its frame -- and the votes for
    its headers; against Vote.new and sanitize_many."""
    from narwhal_amd.crypto import PublicKey, SecretKey, Signer
    from narwhal_amd.messages import Authority, Certificate, Committee, Header, Vote, sanitize_many, sanitize_many_ex
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verify.json")))
    keys = [(PublicKey(bytes.fromhex(p)), SecretKey(bytes.fromhex(s) + bytes.fromhex(p)))
            for s, p in zip(g["reference_keys"]["seeds"], g["reference_keys"]["pks"])]
    committee = Committee({pk: Authority(1, [0]) for pk, _ in keys})
    me, my_secret = keys[0]
    try:
        parents = {c.digest() for c in Certificate.genesis(committee)}
        old = Header.new(me, 1, {}, parents, my_secret)
        new = Header.new(me, 2, {}, parents, my_secret)
        theirs = Header.new(keys[2][0], 2, {}, parents, keys[2][1])
        v_old, v_new = Vote.new(old, keys[1][0], keys[1][1]), Vote.new(new, keys[1][0], keys[1][1])
        msgs = [v_old.to_bytes(), v_new.to_bytes(), theirs.to_bytes(), v_old.to_bytes(), theirs.to_bytes(), b"\x03"]
        states = [(0, old), (0, new), (2, new), (0, new), (3, new), (0, None)]
        with Signer(my_secret) as signer:
            got = sanitize_many_ex(msgs, committee, states=states, signer=signer)
            want_sig = Vote.new(theirs, me, signer).signature
            assert [None if e is None else e.name for e, _, _, _ in got] == [None, None, None, "TooOld", "TooOld",
                                                                            "SerializationError"]
            assert [k for _, _, k, _ in got][:5] == [1, 1, 0, 1, 0]
            assert got[0][1] == v_old.digest() and got[1][1] == v_new.digest() and got[2][1] == theirs.id
            assert [s is not None for _, _, _, s in got] == [False, False, True, False, False, False]
            assert got[2][3] == want_sig == Vote.new(theirs, me, my_secret).signature
            # one state for the whole call, no signer: sanitize_many's answers
            digs = []
            plain = sanitize_many(msgs, committee, 2, new, digests=digs)
            same = sanitize_many_ex(msgs, committee, gc_round=2, target=new)
            assert [None if e is None else e.code for e in plain] == [None if e is None else e.code for e, _, _, _ in same]
            assert [d for _, d, _, _ in same] == digs and all(s is None for _, _, _, s in same)
        assert sanitize_many_ex([], committee) == []
    finally:
        lib.nwc_set_committee(None, 0)
