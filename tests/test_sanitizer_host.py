"""The sanitizer entries and the message mirror's Sanitizer, the parts that need no GPU: argument and
lifecycle errors through the real library, and Sanitizer turning return codes into tuples, DagError
and DeviceError with an injected library."""
import ctypes

import pytest

from narwhal_amd import _lib
from narwhal_amd.crypto import Digest, PublicKey
from narwhal_amd.messages import DagError, Header, Sanitizer


def test_sanitizer_calls_before_init_fail_loudly():
    lib = _lib.load(init=False)
    if lib.nwc_device_count() != 0:
        return   # another test of this process initialised a device: nothing to check here
    assert lib.nwc_sanitizer_create(0, 0) is None
    assert b"nwc_init" in lib.nwc_last_error() and lib.nwc_last_error_code() == _lib.NWC_ERR_NOT_INIT
    # a non-null handle is not touched before the library is initialised
    fake = ctypes.create_string_buffer(64)
    dig, kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
    assert lib.nwc_sanitizer_sanitize(fake, _lib.buf(bytes(8)), 8, 0, None, dig, kind) == _lib.NWC_ERR_NOT_INIT
    assert lib.nwc_sanitizer_sanitize(fake, None, 0, 0, None, None, None) == _lib.NWC_ERR_NOT_INIT
    assert b"nwc_init" in lib.nwc_last_error()
    assert dig.raw == bytes(32) and kind.raw == bytes(1) and fake.raw == bytes(64)


def test_sanitizer_null_arguments_are_argument_errors():
    lib = _lib.load(init=False)
    fake = ctypes.create_string_buffer(64)
    out = (ctypes.c_uint64 * 8)()
    dig, kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
    assert lib.nwc_sanitizer_sanitize(None, _lib.buf(bytes(8)), 8, 0, None, dig, kind) == _lib.NWC_ERR_ARG
    assert lib.nwc_last_error_code() == _lib.NWC_ERR_ARG and lib.nwc_last_error() != b""
    assert lib.nwc_sanitizer_sanitize(None, None, 0, 0, None, None, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_sanitizer_sanitize(fake, None, 8, 0, None, dig, kind) == _lib.NWC_ERR_ARG   # null msg with len > 0
    assert lib.nwc_sanitizer_stats(None, out) == _lib.NWC_ERR_ARG
    assert lib.nwc_sanitizer_stats(fake, None) == _lib.NWC_ERR_ARG
    assert lib.nwc_sanitizer_destroy(None) == _lib.NWC_ERR_ARG
    assert fake.raw == bytes(64) and list(out) == [0] * 8 and dig.raw == bytes(32) and kind.raw == bytes(1)


class _FakeLib:
    """The four sanitizer entries with scripted answers."""

    def __init__(self, code=0, handle=0x1000):
        self.code, self.handle, self.calls, self.destroyed = code, handle, [], 0

    def nwc_sanitizer_create(self, max_messages, max_wait_us):
        self.calls.append(("create", max_messages, max_wait_us))
        return self.handle

    def nwc_sanitizer_sanitize(self, h, msg, n, gc_round, target, dig, kind):
        t = None if target is None else ctypes.string_at(target, 72)
        self.calls.append(("sanitize", h, n, gc_round, t))
        dig[0] = b"\x07"
        kind[0] = b"\x02"
        return self.code

    def nwc_sanitizer_stats(self, h, out):
        for i in range(8):
            out[i] = 20 + i
        return 0

    def nwc_sanitizer_destroy(self, h):
        self.destroyed += 1
        return 0

    def nwc_last_error(self):
        return b"scripted"

    def nwc_last_error_code(self):
        return _lib.NWC_ERR_NOT_INIT


def test_sanitizer_maps_codes_to_tuples_dag_errors_and_device_errors():
    header = Header(author=PublicKey(bytes([5]) * 32), round=9, id=Digest(bytes([3]) * 32))
    with Sanitizer(8, 250, lib=_FakeLib(code=0)) as s:
        fake = s._lib
        assert fake.calls[0] == ("create", 8, 250)
        code, dig, kind = s.sanitize(b"wire", gc_round=4)
        assert (code, kind) == (0, 2) and bytes(dig) == b"\x07" + bytes(31)
        assert fake.calls[-1] == ("sanitize", 0x1000, 4, 4, None)
        assert s.check(b"wire", target=header) == (dig, 2)
        assert fake.calls[-1] == ("sanitize", 0x1000, 4, 0, bytes([3]) * 32 + (9).to_bytes(8, "little") + bytes([5]) * 32)
        assert s.sanitize(b"")[0] == 0 and fake.calls[-1][2] == 0   # a message of no bytes is passed on
        assert s.stats() == dict(zip(Sanitizer.STATS, range(20, 28)))
    assert fake.destroyed == 1
    with Sanitizer(lib=_FakeLib(code=6)) as s:
        assert s.sanitize(b"wire")[0] == 6
        with pytest.raises(DagError) as e:
            s.check(b"wire")
        assert e.value.code == 6 and e.value.name == "CertificateRequiresQuorum"
    with Sanitizer(lib=_FakeLib(code=_lib.NWC_ERR_DEVICE)) as s:
        assert s.sanitize(b"wire")[0] == _lib.NWC_ERR_DEVICE
        with pytest.raises(_lib.DeviceError):   # a device failure is never reported as a DagError
            s.check(b"wire")
    with pytest.raises(_lib.DeviceError):       # create returned NULL
        Sanitizer(lib=_FakeLib(handle=None))


def test_sanitizer_close_is_idempotent():
    fake = _FakeLib()
    s = Sanitizer(lib=fake)
    s.close()
    s.close()
    del s
    assert fake.destroyed == 1
