"""GPU tests of the decoded message views (nwc_sanitize_messages_view, nwc_dev_sanitize_messages_view,
k_message_views).

Every record is compared field for field with the model of tests/msg_view_model.py, which stands
on oracle/messages_ref.py `decode`; codes, digests, kinds and votes are compared byte for byte with
nwc_sanitize_messages_ex on the same arguments.  The committee and the wire fixtures are those of
tests/sanitize_ex_helper.py; the shapes are the smallest at which the kernel takes another path: a
wave's 64 lanes (63, 64, 65), two strides (129, 130), and 600 unsorted entries, above the 512 at
which canon_entries changes from the rank sort to the bitonic network."""
import base64
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import msg_view_model as vm
from tests.conftest import GOLDEN, ROOT
from tests.msg_view_helper import Model, check_views, dev_view, run_view, view_and_ex
from tests.sanitize_ex_helper import SIGNER_KEY, ExWorld, fixture, run_ex, vote_batch
from tests.test_gpu_messages import _install

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HELPER = os.path.join(ROOT, "tests", "msg_view_helper.py")
COUNTS = [0, 1, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def world(lib, oracle):
    from narwhal_amd import _lib
    w = ExWorld(oracle)
    w.install(lib)
    signer = lib.nwc_signer_create(_lib.buf(w.seeds[SIGNER_KEY] + w.pks[SIGNER_KEY]))
    assert signer, lib.nwc_last_error()
    yield w, fixture(w), signer, Model(w.pks)
    assert lib.nwc_signer_destroy(signer) == 0
    lib.nwc_set_committee(None, 0)


# ---- 1. the golden wire fixtures -------------------------------------------------------------------
def test_golden_fixtures_in_one_call_and_one_per_call(lib):
    g = json.load(open(os.path.join(GOLDEN, "messages.json")))
    c = g["committee"]
    keys = [bytes.fromhex(k) for k in c["keys"]]
    _install(lib, keys, c["stakes"], c["workers"])
    try:
        items = []
        for case in g["cases"]:
            t = case["target"]
            items.append((bytes.fromhex(case["msg"]), case["gc_round"], None if t is None else (bytes.fromhex(t[0]), t[1], bytes.fromhex(t[2]))))
        model = Model(keys)
        got, recs = view_and_ex(lib, items, model, what="golden")
        for i, case in enumerate(g["cases"]):
            assert int(got[0][i]) == case["code"], case["name"]
            assert recs[i]["decoded"] == (0 if case["code"] in (8, 10, 11) else 1), case["name"]
        assert any(r["flags"] == 3 for r in recs) and any(r["n_votes"] for r in recs) and got[7] > 0
        for i, it in enumerate(items):
            one, rec = view_and_ex(lib, [it], model, what=g["cases"][i]["name"])
            assert one[5][0][:136].tobytes() == got[5][i][:136].tobytes()   # all but the three offsets
    finally:
        lib.nwc_set_committee(None, 0)


# ---- 2. the smallest shapes at which the kernel can go wrong ------------------------------------------
def _entries(w, n):
    return sorted(w.rand32() for _ in range(n))


def _shuffled(w, ent):
    """The entries with duplicates, in an order that is not ascending (for one entry: twice)."""
    if not ent:
        return []
    out = list(ent) + [ent[0], ent[len(ent) // 2]]
    idx = w.rng.permutation(len(out))
    out = [out[i] for i in idx]
    if all(a < b for a, b in zip(out, out[1:])):
        out.reverse()
    return out


def _message(w, payload, parents, votes=None, key_texts=None, author=0):
    """A header (votes None) or a certificate over the entries in wire order.  The view does not
    depend on the verdict, so the id and the signatures are arbitrary bytes."""
    hdr = w.mr.enc_header(w.pks[author], 4, payload, parents, w.rand32(), bytes(64), wire_order=True)
    if votes is None:
        return w.mr.msg_header(hdr)
    return w.mr.msg_certificate(hdr, votes, key_texts=key_texts)


def _both(w, payload, parents):
    votes = [(w.pks[1], bytes(64)), (w.pks[2], bytes(64))]
    return [(_message(w, payload, parents), 0, None), (_message(w, payload, parents, votes), 0, None)]


def test_ascending_payload_and_parents_stay_in_the_wire(lib, world):
    w, f, signer, model = world
    items = []
    for n in COUNTS:
        items += _both(w, [(d, 0) for d in _entries(w, n)], _entries(w, n))
    got, recs = view_and_ex(lib, items, model, what="ascending")
    for k, r in enumerate(recs):
        n = COUNTS[k // 2]
        assert (r["decoded"], r["flags"], r["n_payload"], r["n_parents"]) == (1, 0, n, n), k
    # nothing but the certificates' voter entries is in the body
    assert got[7] == 16 * len(COUNTS)


def test_shuffled_entries_with_duplicates_go_to_the_body(lib, world):
    w, f, signer, model = world
    items, want = [], []
    for n in COUNTS[1:]:
        dig = _entries(w, n)
        wire = _shuffled(w, dig)
        # worker ids by wire position: the LAST occurrence of a digest decides its value
        payload = [(d, 100 + j) for j, d in enumerate(wire)]
        items += _both(w, payload, _shuffled(w, dig))
        last = {d: wid for d, wid in payload}
        want += [sorted(last.items())] * 2
    got, recs = view_and_ex(lib, items, model, what="shuffled")
    body = got[6].tobytes()
    for k, (r, it) in enumerate(zip(recs, items)):
        n = COUNTS[1:][k // 2]
        assert (r["decoded"], r["flags"], r["n_payload"], r["n_parents"]) == (1, 3, n, n), k
        assert vm.entries(r, it[0], body)[0] == want[k], k


def test_one_sequence_ascending_and_the_other_not(lib, world):
    w, f, signer, model = world
    items = []
    for n in (2, 65, 600):
        dig = _entries(w, n)
        items += _both(w, [(d, 0) for d in dig], _shuffled(w, dig))
        items += _both(w, [(d, 7) for d in _shuffled(w, dig)], dig)
    got, recs = view_and_ex(lib, items, model, what="one of two")
    assert [r["flags"] for r in recs] == [2, 2, 1, 1] * 3
    assert [r["n_payload"] for r in recs] == [2] * 4 + [65] * 4 + [600] * 4


def test_voters_fast_and_slow_path(lib, world):
    w, f, signer, model = world
    items = []
    for V in (1, 63, 64, 65, 130):
        votes = [(w.pks[int(k)], w.rand32() + w.rand32()) for k in w.rng.integers(0, 5, V)]
        items.append((_message(w, [], _entries(w, 2), votes), 0, None))
    # V = 65, vote 64 under a 48-symbol key string: no fixed stride, the parse's voff[] entries
    votes = [(w.pks[v % 5], bytes(64)) for v in range(65)]
    texts = [None] * 65
    texts[64] = base64.b64encode(w.pks[4] + b"\x01\x02\x03\x04")
    assert len(texts[64]) == 48
    items.append((_message(w, [], _entries(w, 3), votes, key_texts=texts), 0, None))
    # ... and with unsorted parents in front of the offsets' place in the scratch slot
    items.append((_message(w, [(w.rand32(), 0)], _shuffled(w, _entries(w, 3)), votes, key_texts=texts), 0, None))
    got, recs = view_and_ex(lib, items, model, what="voters")
    assert [r["n_votes"] for r in recs] == [1, 63, 64, 65, 130, 65, 65]
    slow = vm.entries(recs[5], items[5][0], got[6].tobytes())[2]
    assert slow[64][0] == 4 and slow[64][1] - slow[63][1] == 116 and all(b[1] - a[1] == 116 for a, b in zip(slow, slow[1:]))
    n = struct.unpack_from("<Q", items[5][0], slow[64][1])[0]
    assert n == 48 and slow[64][1] + 8 + 48 + 64 == len(items[5][0])


def test_outsiders_and_messages_that_do_not_decode(lib, world):
    w, f, signer, model = world
    outsider = w.o.public_key(w.rand32())
    hdr, hid = w.header(0, 3, 2)
    cd = w.mr.digest72(hid, 3, w.pks[0])
    cert = w.mr.msg_certificate(hdr, [(w.pks[1], w.o.sign(w.seeds[1], cd)), (outsider, bytes(64)), (w.pks[2], w.o.sign(w.seeds[2], cd))])
    vote = w.vote(2, hid, 7, outsider)
    short = base64.b64encode(w.pks[0][:31])
    panic = w.header_with(0, 5, 1, author_text=short)[0]
    items = [(cert, 0, None), (vote, 0, None), f["truncated"], f["request"], (panic, 0, None), f["empty"]]
    got, recs = view_and_ex(lib, items, model, what="outsiders")
    assert [int(c) for c in got[0]] == [4, 0, 8, 10, 11, 8]        # UnknownAuthority; Ok; the three that do not decode
    assert [r["decoded"] for r in recs] == [1, 1, 0, 0, 0, 0]
    assert [k for k, _ in vm.entries(recs[0], cert, got[6].tobytes())[2]] == [1, -1, 2]
    assert (recs[1]["origin_index"], recs[1]["author_index"], recs[1]["origin"]) == (-1, 2, outsider)
    assert [r["kind"] for r in recs] == [2, 1, 0, 3, 0, 3]
    # the rebuilt objects are the restatement's decode
    for it, r in zip(items[:2], recs[:2]):
        assert vm.rebuild(r, it[0], got[6].tobytes(), w.pks) == w.mr.decode(it[0])


# ---- 3. per-message state and a signer ------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 65])
def test_with_per_message_state_and_a_signer(lib, world, m):
    w, f, signer, model = world
    names = ["hdr-ok", "cert-ok", "vote-ok", "request", "hdr-too-old", "truncated", "vote-stale-target", "hdr-long-key",
             "cert-bad-vote", "hdr-ok-last"]
    items = [f[names[i % len(names)]] for i in range(m)]
    got, recs = view_and_ex(lib, items, model, signer=signer, what="m=%d" % m)
    assert int(got[4][0]) == 1 and (got[3][0] != 0).any()           # the first message is an Ok header: voted
    # without per-message arrays and without a signer: the same views apart from the codes
    plain = run_view(lib, items, own_state=False)
    check_views(items, plain, model, "m=%d plain" % m)


# ---- 4. views == NULL ----------------------------------------------------------------------------------
def _child(mode, env):
    r = subprocess.run([sys.executable, HELPER, mode, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_null_views_is_the_ex_entry(lib, world):
    w, f, signer, model = world
    items = vote_batch(f)
    for sg in (None, signer):
        ex = run_ex(lib, items, sg)
        got = run_view(lib, items, sg, views=False)
        for a, b in zip(ex, got[:5]):
            assert a.tobytes() == b.tobytes()
        assert (got[5] == 0xEE).all() and (got[6] == 0xEE).all() and got[7] == 0xEEEE   # body arguments ignored
    a, b = _child("scratch_ex", {}), _child("scratch_view", {})
    assert a == b and a["scratch"] > 0, (a, b)


# ---- 5. the device entry ---------------------------------------------------------------------------------
def test_device_entry_on_a_side_stream(lib, world):
    import torch
    w, f, signer, model = world
    items = vote_batch(f) + [(_message(w, [(d, 3) for d in _shuffled(w, _entries(w, 5))], _shuffled(w, _entries(w, 4)),
                                       [(w.pks[3], bytes(64))]), 0, None)]
    host = run_view(lib, items, signer)
    rc, got = dev_view(lib, items, signer, torch.cuda.Stream())
    assert rc == 0, lib.nwc_last_error()
    for a, b in zip(got[:5], host[:5]):
        assert a.tobytes() == b.tobytes()
    assert got[7] == host[7] > 0
    check_views(items, got, model, "device")
    rc, plain = dev_view(lib, items, None, torch.cuda.Stream())
    assert rc == 0, lib.nwc_last_error()
    check_views(items, plain, model, "device, no signer")
    assert (plain[3] == 0xEE).all() and (plain[4] == 0xEE).all()


# ---- 6. staged and chunked --------------------------------------------------------------------------------
def test_staged_and_chunked_call():
    got = _child("chunked", {"NWC_MSG_CHUNK": "1048576"})
    print({k: v for k, v in got.items() if k != "cuts"}, got["cuts"])
    cuts = got["cuts"]
    assert (4 << 20) <= got["total"] < (4 << 20) + 65536
    assert len(cuts) >= 4 and cuts[0] == 0 and cuts[-1] == got["m"] and all(c % 64 == 0 for c in cuts[1:-1]), cuts
    assert got["same_as_ex"] == [True] * 3
    assert got["checked"] == got["m"] and got["around_cuts"] == 3 * (len(cuts) - 2)
    assert 0 < got["decoded_around_cuts"] and got["decoded"] > got["m"] // 2
    assert got["in_body"] >= got["m"] // 15 - 1 and got["voters"] > 0 and 0 < got["body_used"] <= got["total"] + 64 * got["m"]


# ---- 7. the Python mirror ---------------------------------------------------------------------------------
def test_mirror_sanitize_many_view(lib):
    """narwhal_amd.messages.sanitize_many_view: the objects it builds from the views equal the objects
    whose to_bytes() made the wires (the mirror encodes; the views are its only decoder), and its
    verdicts are sanitize_many_ex's."""
    from narwhal_amd.crypto import Digest, PublicKey, SecretKey, Signature
    from narwhal_amd.messages import (Authority, Certificate, Committee, Header, Vote, sanitize_many_ex, sanitize_many_view)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verify.json")))
    keys = [(PublicKey(bytes.fromhex(p)), SecretKey(bytes.fromhex(s) + bytes.fromhex(p)))
            for s, p in zip(g["reference_keys"]["seeds"], g["reference_keys"]["pks"])]
    committee = Committee({pk: Authority(1, [0]) for pk, _ in keys})
    rng = np.random.default_rng(11)
    r32 = lambda: Digest(bytes(rng.integers(0, 256, 32, dtype=np.uint8)))  # noqa: E731
    try:
        parents = {c.digest() for c in Certificate.genesis(committee)}
        hdr = Header.new(keys[0][0], 1, {r32(): 0, r32(): 0, r32(): 0}, parents, keys[0][1])
        vote = Vote.new(hdr, keys[1][0], keys[1][1])
        outsider = PublicKey(bytes(rng.integers(0, 256, 32, dtype=np.uint8)))
        cert = Certificate(hdr, [(k, Signature.new(Certificate(hdr).digest(), s)) for k, s in keys[1:]] +
                           [(outsider, Signature())])
        # the same header as a Byzantine peer may send it: parents in descending order, one twice
        ps = sorted(bytes(p) for p in hdr.parents)
        wire = hdr.to_bytes()
        at = wire.index(b"".join(ps))
        byz = wire[:at - 8] + struct.pack("<Q", len(ps) + 1) + b"".join(reversed(ps)) + ps[0] + wire[at + 32 * len(ps):]
        msgs = [hdr.to_bytes(), vote.to_bytes(), cert.to_bytes(), byz, b"\x03\0\0\0", hdr.to_bytes()[:-1]]
        got = sanitize_many_view(msgs, committee)
        assert [o for _, _, _, _, o in got[:4]] == [hdr, vote, cert, hdr]
        assert got[4][4] is None and got[5][4] is None
        ex = sanitize_many_ex(msgs, committee)
        assert [(None if e is None else e.code, d, k, s) for e, d, k, s, _ in got] == \
               [(None if e is None else e.code, d, k, s) for e, d, k, s in ex]
        assert [None if e is None else e.name for e, _, _, _, _ in got] == [None, None, "UnknownAuthority", None,
                                                                           "UnexpectedMessage", "SerializationError"]
    finally:
        lib.nwc_set_committee(None, 0)
