"""Subprocess body of tests/test_gpu_sign.py::test_signing_builds_no_verification_tables: a process
that only signs -- nwc_init, create, sign, destroy -- and the table bytes nwc_memory_info reports
before, during and after."""
import ctypes
import json
import sys

import torch  # noqa: F401  (one HIP runtime: torch's)

sys.path.insert(0, sys.argv[2])
from narwhal_amd import _lib  # noqa: E402
from tests.oracle_lib import load_oracle  # noqa: E402

lib = _lib.load()
orc = load_oracle()
seed = bytes(range(32))
out = {"tables_before": _lib.memory_info()["tables"]}
h = lib.nwc_signer_create(_lib.buf(seed + orc.public_key(seed)))
assert h, lib.nwc_last_error()
sig = ctypes.create_string_buffer(64)
_lib.check(lib.nwc_signer_sign(h, _lib.buf(bytes(32)), sig))
many = ctypes.create_string_buffer(64 * 300)
_lib.check(lib.nwc_signer_sign_many(h, _lib.buf(bytes(32) * 300), 300, many))
out["sig_ok"] = sig.raw == orc.sign(seed, bytes(32)) and many.raw == sig.raw * 300
out["tables_signing"] = _lib.memory_info()["tables"]
out["destroy_rc"] = lib.nwc_signer_destroy(h)
m = _lib.Memory()
out["rc_after_destroy"] = lib.nwc_memory_info(ctypes.byref(m))
out["tables_after"] = int(m.tables)
json.dump(out, open(sys.argv[1], "w"))
