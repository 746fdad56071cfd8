"""The grid probe (tests/hip/grid_probe.hip): its build and its ctypes wrapper, in the manner of
tests/half_probe.py, whose flags and helpers it shares.

One shared library that includes narwhal_amd/csrc/kernels.hip whole and adds entries around
torsion_dlog, ge_mul_l, straus_z, sc_mul128 and resolve_q8, compiled with the library's flags plus
half_probe.EXTRA_FLAGS into tests/cpp/build/libnwc_grid_probe.so.  It embeds a hash of its source, of
kernels.hip, of every csrc header and of the flags; `load()` refuses a library whose hash differs from
the tree's (a stale or missing probe fails the GPU tests, it does not skip them), and `build_probe()`,
which __graft_entry__.build() calls, rebuilds exactly then.  A library of its own, so that the first two
probes and their tests stay as they are.
"""
from __future__ import annotations

import ctypes
import glob
import hashlib
import os
import subprocess

import numpy as np

from tests import half_probe as hp

ROOT = hp.ROOT
SRC = os.path.join(ROOT, "tests", "hip", "grid_probe.hip")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "libnwc_grid_probe.so")
MARK = b"NWC_GRID_PROBE_ID:"

# words per record (in, out) of every entry; probe_record_words() in the library holds the same table
ENTRIES = {"probe_torsion_dlog": (30, 1), "probe_mul_l": (8, 2), "probe_zq": (18, 13), "probe_zq_direct": (12, 13)}
LANE_COUNTS = hp.LANE_COUNTS
ragged = hp.ragged


# ---- build ------------------------------------------------------------------------------------
def probe_sources():
    from narwhal_amd import build as nb
    return [SRC, os.path.join(nb.CSRC, "kernels.hip")] + sorted(glob.glob(os.path.join(nb.CSRC, "*.h")))


def probe_source_id() -> str:
    h = hashlib.sha256(" ".join(f for f in hp.probe_flags() if not f.startswith("-I")).encode())
    for s in probe_sources():
        h.update(os.path.relpath(s, ROOT).encode() + b"\0")
        with open(s, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:20]


def embedded_probe_id(path: str = OUT):
    try:
        blob = open(path, "rb").read()
    except OSError:
        return None
    i = blob.find(MARK)
    if i < 0:
        return None
    return blob[i + len(MARK):blob.find(b"\0", i)].decode(errors="replace")


def probe_up_to_date(path: str = OUT) -> bool:
    return embedded_probe_id(path) == probe_source_id()


def build_probe(out: str = OUT, force: bool = False) -> str:
    from narwhal_amd import build as nb
    if not force and probe_up_to_date(out):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [nb.HIPCC] + hp.probe_flags() + ['-DNWC_PROBE_ID="%s"' % probe_source_id(), "-o", out + ".tmp", SRC]
    subprocess.run(cmd, check=True)
    os.replace(out + ".tmp", out)
    return out


# ---- wrapper ----------------------------------------------------------------------------------
_lib = None


def load():
    """The probe library, or an error: missing and stale both fail (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  first, so the process has one HIP runtime (narwhal_amd/_lib.py)
    if not os.path.exists(OUT):
        raise RuntimeError("%s is missing: run __graft_entry__.build()" % os.path.relpath(OUT, ROOT))
    if not probe_up_to_date():
        raise RuntimeError("%s is stale (embeds %s, sources are %s): run __graft_entry__.build()" % (
            os.path.relpath(OUT, ROOT), embedded_probe_id(), probe_source_id()))
    lib = ctypes.CDLL(OUT)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    lib.probe_record_words.restype = ctypes.c_int
    lib.probe_record_words.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.probe_build_id.restype = ctypes.c_char_p
    assert lib.probe_build_id().decode() == probe_source_id()
    for name, (wi, wo) in ENTRIES.items():
        a, b = ctypes.c_int(), ctypes.c_int()
        assert lib.probe_record_words(name.encode(), ctypes.byref(a), ctypes.byref(b)) == 0, name
        assert (a.value, b.value) == (wi, wo), (name, a.value, b.value)
    _lib = lib
    return lib


def run(name: str, records: np.ndarray) -> np.ndarray:
    """One launch of entry `name` over (n, in_words) records of 32-bit words; (n, out_words) uint32 back."""
    import torch
    lib = load()
    wi, wo = ENTRIES[name]
    rec = np.ascontiguousarray(records)
    assert rec.dtype.itemsize == 4 and rec.ndim == 2 and rec.shape[1] == wi, (name, rec.dtype, rec.shape)
    rec = rec.view(np.uint32)
    n = rec.shape[0]
    assert 0 < n < 1 << 24
    din = torch.from_numpy(rec.view(np.int32).copy()).cuda()
    dout = torch.full((n + 1, wo), 0x5A5A5A5A, dtype=torch.int32, device="cuda")   # one guard record past the end
    rc = getattr(lib, name)(din.data_ptr(), dout.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    out = dout.cpu().numpy().view(np.uint32)
    assert (out[n] == 0x5A5A5A5A).all(), "%s wrote past its last record" % name
    assert not (out[:n] == 0x5A5A5A5A).all(axis=1).any(), "%s left a record unwritten" % name
    return out[:n].copy()


def run_whole_and_ragged(name: str, records: np.ndarray, counts=LANE_COUNTS) -> np.ndarray:
    """The whole record set in one launch (more than one block, a ragged last wave), then the first n
    records alone for every n in `counts`: a short launch must give the same words as the whole one."""
    n = len(records)
    assert n > 256 and n % 64 != 0, (name, n)
    whole = run(name, records)
    for c in counts:
        part = run(name, records[:c])
        assert (part == whole[:c]).all(), "%s: a launch of %d records differs from the whole launch" % (name, c)
    return whole
