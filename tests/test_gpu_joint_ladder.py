"""GPU parity of the joint radix-4 table and ladder of the uncached half-size verify path
(narwhal_amd/csrc/ge_u25519.h: geu_build_joint, geu_joint_ladder; kernels.hip: verify_half in k_verify).

Every verdict comes through device.verify and is held to the C oracle's (strict and batch-leaf):
  * every golden verify case with a 32-byte message (the device entry takes 32-byte digests; the fixture
    has none of 64), against the verdicts recorded in the fixture too;
  * 4,096 device-signed triples mutated over the soak's input classes, as tests/test_gpu_feu.py builds them;
  * crafted triples whose R bytes are the A bytes and whose R is A's negation -- valid signatures among
    them (r = +-a), so the table's P = +-Q entries (the identity and a doubling reached by the unified
    addition) decide accepting verdicts -- and the same with a wrong s;
  * prefixes of 1, 63, 64, 65 and 257 triples with the cold kernel switched off, so that k_verify itself
    runs a partial wave, a full wave, two waves and a second block (a process of its own: libnwc reads
    that switch once);
  * one launch beside a committee cache: the members' equations are decided by the comb kernel, the
    others are listed and run by k_verify's list build of the same uncached branch.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests.conftest import ROOT, GOLDEN

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)


def _golden():
    cases = [c for c in json.load(open(os.path.join(GOLDEN, "ed25519_verify.json")))["cases"] if len(c["msg"]) == 64]
    arrays = tuple(np.stack([np.frombuffer(bytes.fromhex(c[k]), np.uint8) for c in cases]) for k in ("msg", "pk", "sig"))
    return cases, arrays


def _crafted():
    """R = A and R = -A: valid signatures (r = +-a) and the same with s + 1."""
    m, p, s = [], [], []
    for i in range(12):
        seed = hashlib.sha256(b"joint-crafted-%d" % i).digest()
        msg = hashlib.sha256(b"joint-msg-%d" % i).digest()
        a, _ = ref.secret_expand(seed)
        A = ref.pt_mul(a, ref.BASEPOINT)
        pk = ref.compress(A)
        for sign in (1, -1):
            Rb = ref.compress(A if sign > 0 else ref.pt_neg(A))
            assert (Rb == pk) if sign > 0 else (Rb[:31] == pk[:31] and Rb[31] == pk[31] ^ 0x80)
            k = ref.scalar_from_hash(ref.sha512(Rb + pk + msg))
            sc = (sign * a + k * a) % ref.L
            for delta in (0, 1):
                m.append(msg)
                p.append(pk)
                s.append(Rb + ((sc + delta) % ref.L).to_bytes(32, "little"))
    return tuple(np.stack([np.frombuffer(x, np.uint8) for x in col]) for col in (m, p, s))


@pytest.fixture(scope="module")
def triples(oracle):
    import torch
    from narwhal_amd import _lib, device
    from tests.soak import mutate
    _lib.check(_lib.load().nwc_set_committee(None, 0))
    n = 4096
    msgs = device.derive32(b"joint-msg", 0, n)
    pks, sigs = device.keygen_sign(device.derive32(b"joint-seed", 0, n), msgs)
    torch.cuda.synchronize()
    m, p, s = (t.cpu().numpy().copy() for t in (msgs, pks, sigs))
    cases, golden = _golden()
    kind = mutate(np.random.default_rng(4), m, p, s, golden)
    assert len(set(kind.tolist())) == 12                      # every class of the soak is present
    crafted = _crafted()
    # the mutated triples first (so the small prefixes mix the classes), then the crafted, then every golden case
    m, p, s = (np.ascontiguousarray(np.concatenate([a, c, g])) for a, c, g in zip((m, p, s), crafted, golden))
    exp = {True: oracle.strict_many(m, p, s), False: oracle.leaf_many(m, p, s)}
    assert 0.25 * n < exp[True][:n].sum() < 0.6 * n
    nc = len(crafted[0])
    assert exp[True][n:n + nc].tolist() == [True, False] * (nc // 2)     # r = +-a signs; s + 1 does not
    for a in (m, p, s, exp[True], exp[False]):
        a.setflags(write=False)
    return m, p, s, exp, (n, nc, cases)


def _verify(m, p, s, strict):
    import torch
    from narwhal_amd import device
    words = device.verify(torch.tensor(m).cuda(), torch.tensor(p).cuda(), torch.tensor(s).cuda(), strict=strict)
    torch.cuda.synchronize()
    return device.unpack_bits(words, len(p))


def test_golden_mutated_and_crafted_triples(triples):
    m, p, s, exp, (n, nc, cases) = triples
    for strict in (True, False):
        got = _verify(m, p, s, strict)
        assert (got == exp[strict]).all(), (strict, np.nonzero(got != exp[strict])[0][:10])
        recorded = np.array([c["strict" if strict else "leaf"] for c in cases], dtype=bool)
        assert (got[n + nc:] == recorded).all(), (strict, np.nonzero(got[n + nc:] != recorded)[0][:10])


def test_small_sizes_through_k_verify(triples, tmp_path):
    m, p, s, exp, (n, nc, _) = triples
    # the crafted triples in front: the one-lane launch is an accepting R = A equation
    order = np.concatenate([np.arange(n, n + nc), np.arange(n)])[:max(SIZES)]
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, m=m[order], p=p[order], s=s[order])
    env = dict(os.environ)
    env["NWC_COLD"] = "0"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "feu_verify_helper.py"), inp, out, ROOT,
                    ",".join(str(k) for k in SIZES)], env=env, check=True, timeout=300)
    r = np.load(out)
    assert exp[True][order][0]
    for k in SIZES:
        assert (r["s%d" % k] == exp[True][order][:k]).all(), k
        assert (r["l%d" % k] == exp[False][order][:k]).all(), k


def test_list_path_beside_a_committee(triples):
    from narwhal_amd import _lib
    m, p, s, exp, (n, nc, _) = triples
    lib = _lib.load()
    # members: the (unmutated or mutated) keys of every fourth of the first 256 triples; the launch holds
    # those triples and 1,280 others, the crafted ones among them, whose keys the cache does not know
    members = np.ascontiguousarray(np.unique(p[0:256:4], axis=0))
    rows = np.concatenate([np.arange(0, 1024), np.arange(n, n + nc), np.arange(2048, 2048 + 256)])
    in_cache = (p[rows][:, None, :] == members[None, :, :]).all(axis=2).any(axis=1)
    assert 32 <= in_cache.sum() and (~in_cache).sum() >= 1024
    try:
        _lib.check(lib.nwc_set_committee(_lib.buf(members), len(members)))
        got = {strict: _verify(m[rows], p[rows], s[rows], strict) for strict in (True, False)}
    finally:
        _lib.check(lib.nwc_set_committee(None, 0))
    for strict in (True, False):
        want = exp[strict][rows]
        assert (got[strict] == want).all(), (strict, np.nonzero(got[strict] != want)[0][:10])
