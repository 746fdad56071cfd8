"""Signing with a registered key on the GPU (include/nwc.h "signing"; kernels k_sign and
k_sign_wide in narwhal_amd/csrc/sign.h): every signature must equal the CPU oracle's RFC 8032 /
dalek signature byte for byte, through both kernels, the host and the device-resident entries, the
crypto mirror's Signer and SignatureService."""
import ctypes
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.oracle_lib import openssl_verify_many

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257)
PATHS = {"auto": 0, "lane": 1, "wide": 2}


@pytest.fixture(scope="module")
def lib():
    from narwhal_amd import _lib
    lb = _lib.load()
    yield lb
    _lib.diag_set("sign_path", 0)


@pytest.fixture(scope="module")
def seeds(golden_verify):
    """The four reference keypairs' seeds, then all-zero and all-0xFF seeds."""
    return [bytes.fromhex(s) for s in golden_verify["reference_keys"]["seeds"]] + [bytes(32), b"\xff" * 32]


@pytest.fixture(scope="module")
def signers(lib, seeds, oracle):
    from narwhal_amd.crypto import Signer
    sg = [Signer(s + oracle.public_key(s)) for s in seeds]
    yield sg
    for s in sg:
        s.close()


def digests_for(n: int) -> np.ndarray:
    """n digests, fixed per n: random, with all-zero and all-0xFF ones among them (n = 1: three sets)."""
    d = np.random.default_rng(1000 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    if n >= 2:
        d[0] = 0
        d[n - 1] = 0xFF
    return d


_expected = {}


def expected(oracle, seeds, k: int, d: np.ndarray, tag) -> np.ndarray:
    """oracle.sign(seed_k, digest) for every digest of d, computed once per (key, digest set)."""
    if (k, tag) not in _expected:
        _expected[(k, tag)] = np.stack([np.frombuffer(oracle.sign(seeds[k], d[i].tobytes()), np.uint8)
                                        for i in range(d.shape[0])])
    return _expected[(k, tag)]


def host_sign_many(lib, signer, d: np.ndarray) -> np.ndarray:
    from narwhal_amd import _lib
    n = d.shape[0]
    out = np.full((n, 64), 0xAA, np.uint8)
    _lib.check(lib.nwc_signer_sign_many(signer.handle, _lib.buf(d) if n else None, n, _lib.buf(out) if n else None))
    return out


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_oracle(lib, signers, seeds, oracle, n, path):
    from narwhal_amd import _lib
    _lib.diag_set("sign_path", PATHS[path])
    sets = [(n, digests_for(n))]
    if n == 1:
        sets += [("zero", np.zeros((1, 32), np.uint8)), ("ff", np.full((1, 32), 0xFF, np.uint8))]
    for tag, d in sets:
        for k, sg in enumerate(signers):
            got = host_sign_many(lib, sg, d)
            exp = expected(oracle, seeds, k, d, tag)
            assert (got == exp).all(), (n, path, tag, k, np.nonzero((got != exp).any(axis=1))[0][:8])
            pks = np.tile(np.frombuffer(bytes(sg.public_key()), np.uint8), (d.shape[0], 1))
            bits = np.zeros((d.shape[0] + 7) // 8, np.uint8)
            _lib.check(lib.nwc_verify_strict_many(_lib.buf(d), _lib.buf(pks), _lib.buf(got), d.shape[0], _lib.buf(bits)))
            assert np.unpackbits(bits, bitorder="little")[:d.shape[0]].all(), (n, path, tag, k)
            assert openssl_verify_many(d, pks, got).all(), (n, path, tag, k)


@pytest.mark.parametrize("path", ["lane", "wide"])
def test_every_window_and_digit_is_selected(lib, signers, seeds, oracle, path):
    """4,096 digests under one key through each kernel: with 64 windows x 16 digit values, the chance
    that some reachable (window, digit) pair is never selected is below 1024 (15/16)^4096 ~ 1e-112,
    so every table entry and both signs are exercised."""
    import torch
    from narwhal_amd import _lib, device
    _lib.diag_set("sign_path", PATHS[path])
    n = 4096
    d = np.random.default_rng(77).integers(0, 256, (n, 32), dtype=np.uint8)
    if ("cover",) not in _expected:
        _, sigs = oracle.keygen_sign_many(np.tile(np.frombuffer(seeds[0], np.uint8), (n, 1)), d)
        assert sigs[5].tobytes() == oracle.sign(seeds[0], d[5].tobytes())
        _expected[("cover",)] = sigs
    got = device.sign(signers[0], torch.from_numpy(d).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    exp = _expected[("cover",)]
    assert (got == exp).all(), np.nonzero((got != exp).any(axis=1))[0][:8]


@pytest.mark.parametrize("path", ["lane", "wide"])
def test_device_strides_and_empty_call(lib, signers, seeds, oracle, path):
    import torch
    from narwhal_amd import _lib, device
    _lib.diag_set("sign_path", PATHS[path])
    d = digests_for(65)
    dd = torch.from_numpy(d).cuda()
    # msg_stride 32
    got = device.sign(signers[1], dd)
    # msg_stride 0: one digest signed n times
    rep = device.sign(signers[1], dd[3].contiguous(), n=5)
    # n == 0: returns 0, writes nothing
    untouched = torch.full((4, 64), 0xAA, dtype=torch.uint8, device="cuda")
    assert lib.nwc_dev_sign(signers[1].handle, None, 32, 0, None, None) == 0
    assert lib.nwc_dev_sign(signers[1].handle, ctypes.c_void_p(dd.data_ptr()), 32, 0,
                            ctypes.c_void_p(untouched.data_ptr()), None) == 0
    assert lib.nwc_signer_sign_many(signers[1].handle, None, 0, None) == 0
    torch.cuda.synchronize()
    exp = expected(oracle, seeds, 1, d, 65)
    assert (got.cpu().numpy() == exp).all()
    assert (rep.cpu().numpy() == exp[3]).all() and rep.shape == (5, 64)
    assert (untouched.cpu().numpy() == 0xAA).all()
    # any other stride is an argument error, and nothing is launched
    assert lib.nwc_dev_sign(signers[1].handle, ctypes.c_void_p(dd.data_ptr()), 64, 2,
                            ctypes.c_void_p(untouched.data_ptr()), None) == _lib.NWC_ERR_ARG
    torch.cuda.synchronize()
    assert (untouched.cpu().numpy() == 0xAA).all()


def test_keypair_from_seed_and_public_key(lib, signers, seeds, oracle):
    from narwhal_amd import _lib
    for k, s in enumerate(seeds):
        out = ctypes.create_string_buffer(64)
        _lib.check(lib.nwc_keypair_from_seed(_lib.buf(s), out))
        assert out.raw == s + oracle.public_key(s), k
        pk = ctypes.create_string_buffer(32)
        _lib.check(lib.nwc_signer_public_key(signers[k].handle, pk))
        assert pk.raw == oracle.public_key(s), k


def test_create_refuses_a_mismatched_public_half(lib, seeds, oracle):
    from narwhal_amd import _lib
    from narwhal_amd.crypto import Signer
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ed25519_ref
    s = seeds[0]
    pk = oracle.public_key(s)
    flipped = bytes([pk[0] ^ 1]) + pk[1:]
    y = next(y for y in range(2, 64) if ed25519_ref.decompress(y.to_bytes(32, "little")) is None)
    undecodable = y.to_bytes(32, "little")
    for bad in (flipped, pk[:31] + bytes([pk[31] ^ 0x80]), undecodable):
        assert lib.nwc_signer_create(_lib.buf(s + bad)) is None
        assert lib.nwc_last_error_code() == _lib.NWC_ERR_ARG
        assert lib.nwc_last_error() != b""
        with pytest.raises(_lib.DeviceError):
            Signer(s + bad)
    # the right half still registers afterwards
    with Signer(s + pk) as sg:
        assert sg.sign(bytes(32)).flatten() == oracle.sign(s, bytes(32))


def test_two_signers_never_mix_keys(lib, signers, seeds, oracle):
    from narwhal_amd import _lib
    _lib.diag_set("sign_path", 0)
    d = digests_for(2)
    for rnd in range(8):
        for k in (2, 3, 2, 3):
            msg = d[rnd & 1].tobytes()
            assert signers[k].sign(msg).flatten() == oracle.sign(seeds[k], msg), (rnd, k)


def test_threads_share_one_signer(lib, signers, seeds, oracle):
    from narwhal_amd import _lib
    _lib.diag_set("sign_path", 0)
    d = np.random.default_rng(5).integers(0, 256, (8, 32, 32), dtype=np.uint8)
    got = [[None] * 32 for _ in range(8)]

    def work(t):
        for i in range(32):
            got[t][i] = signers[0].sign(d[t, i].tobytes()).flatten()

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(8):
        for i in range(32):
            assert got[t][i] == oracle.sign(seeds[0], d[t, i].tobytes()), (t, i)


def test_signature_service_on_the_gpu(lib, seeds, oracle):
    from narwhal_amd.crypto import Digest, SecretKey, SignatureService
    s = seeds[1]
    d = np.random.default_rng(6).integers(0, 256, (4, 64, 32), dtype=np.uint8)
    got = [[None] * 64 for _ in range(4)]
    with SignatureService(SecretKey(s + oracle.public_key(s))) as svc:
        def work(t):
            for i in range(64):
                got[t][i] = svc.request_signature(Digest(d[t, i].tobytes())).flatten()

        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        st = svc.stats()
    assert st["requests"] == 256 and 1 <= st["launches"] <= 256, st
    for t in range(4):
        for i in range(64):
            assert got[t][i] == oracle.sign(s, d[t, i].tobytes()), (t, i)


def test_signing_builds_no_verification_tables(tmp_path):
    """A fresh process that only signs: nwc_init, create, sign, destroy."""
    out = tmp_path / "out.json"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sign_footprint_helper.py"), str(out), ROOT],
                   check=True, timeout=300)
    got = json.load(open(out))
    assert got["tables_before"] == 0
    assert 0 < got["tables_signing"] < (1 << 20), got
    assert got["tables_after"] < (1 << 20) and got["rc_after_destroy"] == 0, got
    assert got["sig_ok"] and got["destroy_rc"] == 0, got


def test_mirror_signature_new_is_unchanged(lib, seeds, oracle):
    from narwhal_amd.crypto import Digest, PublicKey, SecretKey, Signature, Signer
    s = seeds[2]
    sk = SecretKey(s + oracle.public_key(s))
    digest = Digest(digests_for(2)[1].tobytes())
    sig = Signature.new(digest, sk)
    sig.verify(digest, PublicKey(oracle.public_key(s)))
    with Signer(sk) as sg:
        assert sg.sign(digest) == sig
        assert sg.sign_many([digest, Digest()])[0] == sig
