"""The five Vote::new entries of include/nwc.h without a device: they are exported with the
signatures narwhal_amd/_lib.py binds, answer NWC_ERR_NOT_INIT before nwc_init and NWC_ERR_ARG for
null pointers.  The calls run in a child process that never calls nwc_init (this process may have
initialised the library for other tests)."""
import ctypes
import json
import os
import re
import subprocess
import sys

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "nwc.h")
LIB = os.path.join(ROOT, "narwhal_amd", "libnwc.so")
ENTRIES = ("nwc_signer_vote", "nwc_signer_vote_many", "nwc_dev_vote", "nwc_sanitizer_sanitize_vote",
           "nwc_sanitizer_vote_stats")

# C parameter type -> what _lib.py binds it as
CTYPES = {"void*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p,
          "uint8_t*": ctypes.c_void_p, "const uint64_t*": ctypes.c_void_p, "uint64_t": ctypes.c_uint64,
          "size_t": ctypes.c_size_t, "uint64_t*": ctypes.POINTER(ctypes.c_uint64), "int32_t*": ctypes.POINTER(ctypes.c_int32)}


def _header_params(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        q = re.match(r"(const )?(\w+)\s*(\*?)\s*\w+(\[\d+\])?$", " ".join(p.split()))
        assert q, p
        out.append((q.group(1) or "") + q.group(2) + ("*" if q.group(3) or q.group(4) else ""))
    return out


def test_the_five_entries_are_exported_with_the_bound_signatures():
    from narwhal_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in ENTRIES:
        assert name in exported, name
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int, name
        assert args == [CTYPES[t] for t in _header_params(name)], (name, _header_params(name))
    lib = _lib.load(init=False)
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib._SIGS[name][1]


CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from narwhal_amd import _lib
lib = _lib.load(init=False)
z = ctypes.create_string_buffer(256)
p = ctypes.cast(z, ctypes.c_void_p)
h = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)   # stands for a handle: never read before nwc_init
r = (ctypes.c_uint64 * 4)()
voted = ctypes.c_int32(7)
a, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
out = {"not_init": {}, "arg": {}}
ni = out["not_init"]
ni["nwc_signer_vote"] = lib.nwc_signer_vote(h, p, 5, p, p)
ni["nwc_signer_vote_many"] = lib.nwc_signer_vote_many(h, p, r, p, 2, p)
ni["nwc_signer_vote_many_n0"] = lib.nwc_signer_vote_many(h, None, None, None, 0, None)
ni["nwc_dev_vote"] = lib.nwc_dev_vote(h, p, p, p, 2, p, None)
ni["nwc_sanitizer_sanitize_vote"] = lib.nwc_sanitizer_sanitize_vote(h, h, p, 100, 0, None, None, None, p, ctypes.byref(voted))
ni["voted"] = voted.value
ni["nwc_sanitizer_vote_stats"] = lib.nwc_sanitizer_vote_stats(h, ctypes.byref(a), ctypes.byref(b))
ni["message"] = lib.nwc_last_error().decode()
ar = out["arg"]
ar["vote_null_signer"] = lib.nwc_signer_vote(None, p, 5, p, p)
ar["vote_null_id"] = lib.nwc_signer_vote(h, None, 5, p, p)
ar["vote_null_origin"] = lib.nwc_signer_vote(h, p, 5, None, p)
ar["vote_null_sig"] = lib.nwc_signer_vote(h, p, 5, p, None)
ar["many_null_signer"] = lib.nwc_signer_vote_many(None, p, r, p, 2, p)
ar["many_null_ids"] = lib.nwc_signer_vote_many(h, None, r, p, 2, p)
ar["many_null_rounds"] = lib.nwc_signer_vote_many(h, p, None, p, 2, p)
ar["many_null_origins"] = lib.nwc_signer_vote_many(h, p, r, None, 2, p)
ar["many_null_sigs"] = lib.nwc_signer_vote_many(h, p, r, p, 2, None)
ar["dev_null_signer"] = lib.nwc_dev_vote(None, p, p, p, 2, p, None)
ar["dev_null_ids"] = lib.nwc_dev_vote(h, None, p, p, 2, p, None)
ar["dev_null_rounds"] = lib.nwc_dev_vote(h, p, None, p, 2, p, None)
ar["dev_null_origins"] = lib.nwc_dev_vote(h, p, p, None, 2, p, None)
ar["dev_null_sigs"] = lib.nwc_dev_vote(h, p, p, p, 2, None, None)
ar["sv_null_sanitizer"] = lib.nwc_sanitizer_sanitize_vote(None, h, p, 100, 0, None, None, None, p, ctypes.byref(voted))
ar["sv_null_signer"] = lib.nwc_sanitizer_sanitize_vote(h, None, p, 100, 0, None, None, None, p, ctypes.byref(voted))
ar["sv_null_msg"] = lib.nwc_sanitizer_sanitize_vote(h, h, None, 100, 0, None, None, None, p, ctypes.byref(voted))
ar["sv_null_sig"] = lib.nwc_sanitizer_sanitize_vote(h, h, p, 100, 0, None, None, None, None, ctypes.byref(voted))
ar["sv_null_voted"] = lib.nwc_sanitizer_sanitize_vote(h, h, p, 100, 0, None, None, None, p, None)
ar["stats_null_sanitizer"] = lib.nwc_sanitizer_vote_stats(None, ctypes.byref(a), ctypes.byref(b))
ar["code"] = lib.nwc_last_error_code()
out["stats_untouched"] = [a.value, b.value]
print(json.dumps(out))
"""


def test_before_init_and_null_pointers():
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    from narwhal_amd import _lib
    out = json.loads(r.stdout.strip().splitlines()[-1])
    ni = out["not_init"]
    for name in ENTRIES:
        assert ni[name] == _lib.NWC_ERR_NOT_INIT, (name, ni)
    assert ni["nwc_signer_vote_many_n0"] == _lib.NWC_ERR_NOT_INIT   # n == 0 is a no-op only on an initialised library
    assert ni["voted"] == 0 and "nwc_init" in ni["message"], ni
    for what, rc in out["arg"].items():
        if what != "code":
            assert rc == _lib.NWC_ERR_ARG, (what, rc)
    assert out["arg"]["code"] == _lib.NWC_ERR_ARG
    assert out["stats_untouched"] == [7, 7]
