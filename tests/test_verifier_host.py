"""The verifier entries and the crypto mirror's Verifier, the parts that need no GPU: argument and
lifecycle errors through the real library, and Verifier turning return codes into CryptoError /
DeviceError with an injected library."""
import ctypes

import pytest

from narwhal_amd import _lib
from narwhal_amd.crypto import CryptoError, DeviceError, Digest, PublicKey, Signature, Verifier


def test_verifier_calls_before_init_fail_loudly():
    lib = _lib.load(init=False)
    if lib.nwc_device_count() != 0:
        return   # another test of this process initialised a device: nothing to check here
    assert lib.nwc_verifier_create(0, 0) is None
    assert b"nwc_init" in lib.nwc_last_error() and lib.nwc_last_error_code() == _lib.NWC_ERR_NOT_INIT
    # a non-null handle is not touched before the library is initialised
    fake = ctypes.create_string_buffer(64)
    msg, pk, sig = _lib.buf(bytes(32)), _lib.buf(bytes(32)), _lib.buf(bytes(64))
    bitmap = ctypes.create_string_buffer(1)
    assert lib.nwc_verifier_verify_strict(fake, msg, pk, sig) == _lib.NWC_ERR_NOT_INIT
    assert lib.nwc_verifier_verify_batch(fake, msg, pk, sig, 1, bitmap) == _lib.NWC_ERR_NOT_INIT
    assert b"nwc_init" in lib.nwc_last_error()
    assert bitmap.raw == bytes(1) and fake.raw == bytes(64)


def test_verifier_null_arguments_are_argument_errors():
    lib = _lib.load(init=False)
    fake = ctypes.create_string_buffer(64)
    msg, pk, sig = _lib.buf(bytes(32)), _lib.buf(bytes(32)), _lib.buf(bytes(64))
    out = (ctypes.c_uint64 * 8)()
    assert lib.nwc_verifier_verify_strict(None, msg, pk, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_last_error_code() == _lib.NWC_ERR_ARG and lib.nwc_last_error() != b""
    assert lib.nwc_verifier_verify_strict(fake, None, pk, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_strict(fake, msg, None, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_strict(fake, msg, pk, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_batch(None, msg, pk, sig, 1, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_batch(None, msg, pk, sig, 0, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_batch(fake, None, pk, sig, 1, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_batch(fake, msg, None, sig, 1, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_verify_batch(fake, msg, pk, None, 1, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_stats(None, out) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_stats(fake, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_verifier_destroy(None) == _lib.NWC_ERR_ARG
    assert fake.raw == bytes(64) and list(out) == [0] * 8


class _FakeLib:
    """The five verifier entries with scripted answers."""

    def __init__(self, rc=0, bad=()):
        self.rc, self.bad, self.calls, self.destroyed = rc, bad, [], 0

    def nwc_verifier_create(self, max_requests, max_wait_us):
        self.calls.append(("create", max_requests, max_wait_us))
        return 0x1000

    def nwc_verifier_verify_strict(self, h, msg, pk, sig):
        self.calls.append(("strict", h))
        return self.rc

    def nwc_verifier_verify_batch(self, h, msg, pks, sigs, n, bitmap):
        self.calls.append(("batch", h, n))
        for i in self.bad:
            bitmap[i >> 3] = bytes([bitmap[i >> 3][0] | (1 << (i & 7))])
        return self.rc

    def nwc_verifier_stats(self, h, out):
        for i in range(8):
            out[i] = 10 + i
        return 0

    def nwc_verifier_destroy(self, h):
        self.destroyed += 1
        return 0


def _vote(i):
    return PublicKey(bytes([i]) * 32), Signature.from_bytes(bytes([i]) * 64)


def test_verifier_raises_crypto_error_for_invalid_and_device_error_for_failures():
    digest = Digest(bytes(32))
    pk, sig = _vote(1)
    with Verifier(8, 250, lib=_FakeLib(rc=_lib.NWC_OK)) as v:
        assert v._lib.calls[0] == ("create", 8, 250)
        v.verify(digest, pk, sig)
        v.verify_batch(digest, [_vote(1), _vote(2)])
        v.verify_batch(digest, [])
        assert v.stats() == dict(zip(Verifier.STATS, range(10, 18)))
        fake = v._lib
    assert fake.destroyed == 1
    with Verifier(lib=_FakeLib(rc=_lib.NWC_INVALID, bad=(0, 9))) as v:
        with pytest.raises(CryptoError):
            v.verify(digest, pk, sig)
        bad = []
        with pytest.raises(CryptoError):
            v.verify_batch(digest, [_vote(i) for i in range(10)], bad=bad)
        assert bad == [0, 9]
    with Verifier(lib=_FakeLib(rc=_lib.NWC_ERR_DEVICE)) as v:
        with pytest.raises(DeviceError):   # a device failure is never reported as an invalid signature
            v.verify(digest, pk, sig)
        with pytest.raises(DeviceError):
            v.verify_batch(digest, [_vote(3)])
    with pytest.raises(ValueError):
        Verifier(lib=_FakeLib()).verify(b"short", pk, sig)


def test_verifier_close_is_idempotent():
    fake = _FakeLib()
    v = Verifier(lib=fake)
    v.close()
    v.close()
    del v
    assert fake.destroyed == 1
