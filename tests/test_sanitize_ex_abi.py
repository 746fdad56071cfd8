"""nwc_sanitize_messages_ex / nwc_dev_sanitize_messages_ex without a device (include/nwc.h): the
library exports both, and their argument conventions answer before anything touches a GPU.

The calls run in a fresh process that never calls nwc_init (another test of this process may have):
  - a signer with NULL vote outputs is NWC_ERR_ARG, whatever else is passed (the signer pointer is
    not dereferenced for that);
  - m == 0 is a no-op returning 0;
  - every other call before nwc_init is NWC_ERR_NOT_INIT, and the host entry has then zeroed the
    vote outputs ("on an error < 0 every vote output is zero").
"""
import json
import os
import subprocess
import sys

from tests.conftest import ROOT

LIB = os.path.join(ROOT, "narwhal_amd", "libnwc.so")

CHILD = r'''
import ctypes, json, sys
sys.path.insert(0, %r)
from narwhal_amd import _lib
lib = _lib.load(init=False)
out = {}
data = bytes(8)
offs = (ctypes.c_uint64 * 2)(0, 8)
codes = (ctypes.c_int32 * 1)(77)
sigs = ctypes.create_string_buffer(b"\xff" * 64, 64)
voted = ctypes.create_string_buffer(b"\xff", 1)
fake = ctypes.c_void_p(0x1000)   # never dereferenced: the argument check comes first
p = _lib.buf(data)
out["host_not_init"] = lib.nwc_sanitize_messages_ex(p, offs, 1, None, 0, None, None, None, codes, None, None, None, None)
out["host_not_init_code"] = lib.nwc_last_error_code()
out["host_not_init_text"] = lib.nwc_last_error().decode()
out["dev_not_init"] = lib.nwc_dev_sanitize_messages_ex(p, p, 1, 8, None, 0, None, None, None, p, None, None, None, None, None)
out["host_signer_null_outputs"] = [
    lib.nwc_sanitize_messages_ex(p, offs, 1, None, 0, None, None, fake, codes, None, None, None, voted),
    lib.nwc_sanitize_messages_ex(p, offs, 1, None, 0, None, None, fake, codes, None, None, sigs, None),
    lib.nwc_sanitize_messages_ex(p, offs, 0, None, 0, None, None, fake, codes, None, None, None, None)]
out["dev_signer_null_outputs"] = [
    lib.nwc_dev_sanitize_messages_ex(p, p, 1, 8, None, 0, None, None, fake, p, None, None, None, p, None),
    lib.nwc_dev_sanitize_messages_ex(p, p, 1, 8, None, 0, None, None, fake, p, None, None, p, None, None)]
out["arg_code"] = lib.nwc_last_error_code()
sigs = ctypes.create_string_buffer(b"\xff" * 64, 64)   # (the refused calls above may have zeroed theirs)
voted = ctypes.create_string_buffer(b"\xff", 1)
out["m0"] = [lib.nwc_sanitize_messages_ex(None, None, 0, None, 0, None, None, None, None, None, None, None, None),
             lib.nwc_sanitize_messages_ex(None, None, 0, None, 0, None, None, fake, None, None, None, sigs, voted),
             lib.nwc_dev_sanitize_messages_ex(None, None, 0, 0, None, 0, None, None, None, None, None, None, None, None, None)]
out["m0_untouched"] = sigs.raw == b"\xff" * 64 and voted.raw == b"\xff"
# a signer and its outputs before nwc_init: NOT_INIT, and the vote outputs are zero
out["host_signer_not_init"] = lib.nwc_sanitize_messages_ex(p, offs, 1, None, 0, None, None, fake, codes, None, None, sigs, voted)
out["zeroed"] = sigs.raw == bytes(64) and voted.raw == bytes(1)
out["codes_untouched"] = codes[0] == 77
print(json.dumps(out))
'''


def _nm():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_library_exports_both_entries():
    assert {"nwc_sanitize_messages_ex", "nwc_dev_sanitize_messages_ex"} <= _nm()


def test_conventions_before_init():
    from narwhal_amd import _lib
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["host_not_init"] == _lib.NWC_ERR_NOT_INIT and got["host_not_init_code"] == _lib.NWC_ERR_NOT_INIT, got
    assert "nwc_init" in got["host_not_init_text"], got
    assert got["dev_not_init"] == _lib.NWC_ERR_NOT_INIT, got
    assert got["host_signer_null_outputs"] == [_lib.NWC_ERR_ARG] * 3, got
    assert got["dev_signer_null_outputs"] == [_lib.NWC_ERR_ARG] * 2 and got["arg_code"] == _lib.NWC_ERR_ARG, got
    assert got["m0"] == [0, 0, 0] and got["m0_untouched"], got
    assert got["host_signer_not_init"] == _lib.NWC_ERR_NOT_INIT and got["zeroed"] and got["codes_untouched"], got
