"""Signing through the C ABI and the crypto mirror, the parts that need no GPU: argument and
lifecycle errors of the signer entries, and the SignatureService queue with an injected signer."""
import ctypes
import threading

from narwhal_amd import _lib
from narwhal_amd.crypto import Signature, SignatureService


def test_signer_calls_before_init_fail_loudly():
    lib = _lib.load(init=False)
    if lib.nwc_device_count() != 0:
        return   # another test of this process initialised a device: nothing to check here
    seed, out = _lib.buf(bytes(32)), ctypes.create_string_buffer(64)
    assert lib.nwc_keypair_from_seed(seed, out) == _lib.NWC_ERR_NOT_INIT
    assert b"nwc_init" in lib.nwc_last_error()
    assert lib.nwc_last_error_code() == _lib.NWC_ERR_NOT_INIT
    assert out.raw == bytes(64)
    assert lib.nwc_signer_create(_lib.buf(bytes(64))) is None
    assert b"nwc_init" in lib.nwc_last_error() and lib.nwc_last_error_code() == _lib.NWC_ERR_NOT_INIT
    # a non-null handle is not touched before the library is initialised
    fake = ctypes.create_string_buffer(64)
    sig = ctypes.create_string_buffer(64)
    assert lib.nwc_signer_sign(fake, seed, sig) == _lib.NWC_ERR_NOT_INIT
    assert lib.nwc_signer_sign_many(fake, seed, 1, sig) == _lib.NWC_ERR_NOT_INIT
    assert lib.nwc_dev_sign(fake, fake, 32, 1, sig, None) == _lib.NWC_ERR_NOT_INIT
    assert sig.raw == bytes(64)


def test_signer_null_arguments_are_argument_errors():
    lib = _lib.load(init=False)
    msg, sig = _lib.buf(bytes(32)), ctypes.create_string_buffer(64)
    assert lib.nwc_signer_create(None) is None
    assert lib.nwc_last_error_code() == _lib.NWC_ERR_ARG and lib.nwc_last_error() != b""
    assert lib.nwc_keypair_from_seed(None, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_keypair_from_seed(msg, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_sign(None, msg, sig) == _lib.NWC_ERR_ARG
    fake = ctypes.create_string_buffer(64)
    assert lib.nwc_signer_sign(fake, None, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_sign(fake, msg, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_sign_many(None, msg, 1, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_sign_many(fake, None, 1, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_sign_many(fake, msg, 1, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_dev_sign(None, msg, 32, 1, sig, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_dev_sign(fake, None, 32, 1, sig, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_public_key(None, sig) == _lib.NWC_ERR_ARG
    assert lib.nwc_signer_destroy(None) == _lib.NWC_ERR_ARG
    assert sig.raw == bytes(64)


def test_sign_path_knob_range():
    lib = _lib.load(init=False)
    assert lib.nwc_diag_set(b"sign_path", 3) == _lib.NWC_ERR_ARG
    for v in (1, 2, 0):
        assert lib.nwc_diag_set(b"sign_path", v) == 0
    assert lib.nwc_version() == (1 << 16) | 2


class _BlockingSigner:
    """sign_many records its batch, waits for `release`, and answers digest || digest."""

    def __init__(self):
        self.release = threading.Event()
        self.entered = threading.Event()
        self.batches = []

    def sign_many(self, digests):
        self.batches.append(list(digests))
        self.entered.set()
        assert self.release.wait(30)
        return [Signature.from_bytes(bytes(d) * 2) for d in digests]


def test_signature_service_coalesces_requests_behind_a_launch():
    fake = _BlockingSigner()
    svc = SignatureService(signer=fake)
    results = {}

    def ask(i):
        results[i] = svc.request_signature(bytes([i]) * 32)

    first = threading.Thread(target=ask, args=(0,))
    first.start()
    assert fake.entered.wait(30)          # launch 1 (one request) is in flight and blocked
    rest = [threading.Thread(target=ask, args=(i,)) for i in range(1, 11)]
    for t in rest:
        t.start()
    # all ten are queued behind the blocked launch before it is released
    deadline = threading.Event()
    while svc.stats()["requests"] < 11:
        assert not deadline.wait(0.001)
    assert svc.stats() == {"requests": 11, "launches": 1}
    fake.release.set()
    for t in [first] + rest:
        t.join(30)
        assert not t.is_alive()
    svc.close()
    assert [len(b) for b in fake.batches] == [1, 10]
    assert svc.stats() == {"requests": 11, "launches": 2}
    for i in range(11):
        assert results[i].flatten() == bytes([i]) * 64     # every caller got its own signature


def test_signature_service_hands_a_signer_error_to_its_callers():
    class Broken:
        def sign_many(self, digests):
            raise _lib.DeviceError("device lost")

    with SignatureService(signer=Broken()) as svc:
        try:
            svc.request_signature(bytes(32))
            raise AssertionError("no error")
        except _lib.DeviceError as e:
            assert "device lost" in str(e)
        assert svc.stats() == {"requests": 1, "launches": 1}
