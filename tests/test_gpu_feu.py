"""GPU parity of the uncached half-size verify path on the non-negative field (fe_u25519.h,
ge_u25519.h; kernels.hip: verify_half's uncached branch in k_verify).

One set of inputs, one oracle evaluation shared by every test: every golden verify case and 4,096
device-signed triples mutated over the soak's input classes (tests/soak.py: bit flips in R, s, A and
the message, s + l, small-order and non-canonical encodings, random bytes, the golden cases tiled
in).  The device entry's strict and leaf verdicts must equal the C oracle's
  * on the whole set (more than one block, a ragged last wave);
  * with each window count W = 33..37 forced through the force_windows diagnostic;
  * on prefixes of 1, 63, 64, 65, 255, 256 and 257 triples with the cold kernel switched off, so
    that k_verify itself runs them (a partial wave, one wave, one lane past it, one block, ...);
  * with every third equation sent through the fallback hook.
The last two run in a process of their own each: libnwc reads those switches once.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, GOLDEN

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def triples(oracle):
    import torch
    from narwhal_amd import _lib, device
    from tests.soak import mutate
    _lib.check(_lib.load().nwc_set_committee(None, 0))
    n = 4096
    msgs = device.derive32(b"feu-msg", 0, n)
    pks, sigs = device.keygen_sign(device.derive32(b"feu-seed", 0, n), msgs)
    torch.cuda.synchronize()
    m, p, s = (t.cpu().numpy().copy() for t in (msgs, pks, sigs))
    cases = [c for c in json.load(open(os.path.join(GOLDEN, "ed25519_verify.json")))["cases"] if len(c["msg"]) == 64]
    golden = tuple(np.stack([np.frombuffer(bytes.fromhex(c[k]), np.uint8) for c in cases]) for k in ("msg", "pk", "sig"))
    kind = mutate(np.random.default_rng(25519), m, p, s, golden)
    assert len(set(kind.tolist())) == 12                      # every class of the soak is present
    # the mutated triples first (so the small prefixes mix the classes), then every golden case
    m, p, s = (np.ascontiguousarray(np.concatenate([a, g])) for a, g in zip((m, p, s), golden))
    exp = {True: oracle.strict_many(m, p, s), False: oracle.leaf_many(m, p, s)}
    assert 0.25 * n < exp[True].sum() < 0.6 * n
    for a in (m, p, s, exp[True], exp[False]):
        a.setflags(write=False)
    return m, p, s, exp


def _verify(m, p, s, strict):
    import torch
    from narwhal_amd import device
    words = device.verify(torch.tensor(m).cuda(), torch.tensor(p).cuda(), torch.tensor(s).cuda(), strict=strict)
    torch.cuda.synchronize()
    return device.unpack_bits(words, len(p))


def test_golden_and_mutated_triples(triples):
    m, p, s, exp = triples
    for strict in (True, False):
        got = _verify(m, p, s, strict)
        assert (got == exp[strict]).all(), (strict, np.nonzero(got != exp[strict])[0][:10])


@pytest.mark.parametrize("W", [33, 34, 35, 36, 37])
def test_forced_window_counts(triples, W):
    from narwhal_amd import _lib
    m, p, s, exp = triples
    _lib.diag_set("force_windows", W)
    try:
        got = {strict: _verify(m, p, s, strict) for strict in (True, False)}
    finally:
        _lib.diag_set("force_windows", 0)
    for strict in (True, False):
        assert (got[strict] == exp[strict]).all(), (W, strict, np.nonzero(got[strict] != exp[strict])[0][:10])


def _child(triples, tmp_path, env_extra, sizes):
    m, p, s, _ = triples
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, m=m, p=p, s=s)
    env = dict(os.environ)
    env.update(env_extra)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "feu_verify_helper.py"), inp, out, ROOT,
                    ",".join(str(n) for n in sizes)], env=env, check=True, timeout=300)
    return np.load(out)


def test_small_sizes_through_k_verify(triples, tmp_path):
    exp = triples[3]
    r = _child(triples, tmp_path, {"NWC_COLD": "0"}, SIZES)
    for n in SIZES:
        assert (r["s%d" % n] == exp[True][:n]).all(), n
        assert (r["l%d" % n] == exp[False][:n]).all(), n


def test_fallback_hook(triples, tmp_path):
    exp = triples[3]
    n = len(exp[True])
    r = _child(triples, tmp_path, {"NWC_FORCE_FALLBACK_EVERY": "3"}, (n,))
    assert (r["s%d" % n] == exp[True]).all(), np.nonzero(r["s%d" % n] != exp[True])[0][:10]
    assert (r["l%d" % n] == exp[False]).all(), np.nonzero(r["l%d" % n] != exp[False])[0][:10]
