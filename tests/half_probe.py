"""The half-size probe (tests/hip/half_probe.hip): its build and its ctypes wrapper, in the manner of
tests/prim_probe.py.

One shared library that includes narwhal_amd/csrc/kernels.hip whole and adds entries around
lat::reduce, challenge, base_digits, the recodings, the window counts and the two half-size ladders,
compiled with the library's flags (narwhal_amd.build.FLAGS) plus EXTRA_FLAGS into
tests/cpp/build/libnwc_half_probe.so.  It embeds a hash of its source, of kernels.hip, of every csrc
header and of the flags; `load()` refuses a library whose hash differs from the tree's (a stale or
missing probe fails the GPU tests, it does not skip them), and `build_probe()` rebuilds exactly then.
"""
from __future__ import annotations

import ctypes
import glob
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hip", "half_probe.hip")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "libnwc_half_probe.so")
MARK = b"NWC_HALF_PROBE_ID:"

# The translation unit holds every kernel of kernels.hip under the library's own names.  Host side
# only: its symbols stay out of the dynamic table and its own references bind inside the library, so
# it loads beside libnwc.so without either seeing the other's.  The device code is compiled with
# exactly the library's flags.
EXTRA_FLAGS = ["-Xarch_host", "-fvisibility=hidden", "-Wl,-Bsymbolic"]

# words per record (in, out) of every entry; probe_record_words() in the library holds the same table
ENTRIES = {
    "probe_lat_reduce": (8, 13), "probe_challenge": (24, 16), "probe_base_digits": (13, 31),
    "probe_half_recode": (7, 182), "probe_wave_windows": (1, 2),
    "probe_half_ladder_u": (35, 33), "probe_half_ladder_cached": (28, 33),
}
LADDERS = ("probe_half_ladder_u", "probe_half_ladder_cached")
PAR_WORDS = 8
SLOT_BYTES = 2304        # 2 * TAB_BYTES_PER_LANE
LANE_COUNTS = (1, 63, 64, 65)
UNUSED = 0x7777          # probe_half_recode: a slot past a string's length


# ---- build ------------------------------------------------------------------------------------
def probe_sources():
    from narwhal_amd import build as nb
    return [SRC, os.path.join(nb.CSRC, "kernels.hip")] + sorted(glob.glob(os.path.join(nb.CSRC, "*.h")))


def probe_flags():
    from narwhal_amd import build as nb
    return nb.FLAGS + EXTRA_FLAGS


def probe_source_id() -> str:
    h = hashlib.sha256(" ".join(f for f in probe_flags() if not f.startswith("-I")).encode())
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
    """hipcc with the library's own flags; rebuilt when the probe source, kernels.hip, a csrc header or
    a flag changed."""
    from narwhal_amd import build as nb
    if not force and probe_up_to_date(out):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [nb.HIPCC] + probe_flags() + ['-DNWC_PROBE_ID="%s"' % probe_source_id(), "-o", out + ".tmp", SRC]
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
        fn.argtypes = [ctypes.c_void_p] * (3 if name in LADDERS else 2) + [ctypes.c_uint32, ctypes.c_void_p]
    lib.probe_record_words.restype = ctypes.c_int
    lib.probe_record_words.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.probe_build_id.restype = ctypes.c_char_p
    assert lib.probe_build_id().decode() == probe_source_id()
    for name, (wi, wo) in ENTRIES.items():
        a, b = ctypes.c_int(), ctypes.c_int()
        assert lib.probe_record_words(name.encode(), ctypes.byref(a), ctypes.byref(b)) == 0, name
        assert (a.value, b.value) == (wi, wo), (name, a.value, b.value)
    assert lib.probe_ladder_par_words() == PAR_WORDS and lib.probe_ladder_slot_bytes() == SLOT_BYTES
    _lib = lib
    return lib


def run(name: str, records: np.ndarray, par: np.ndarray = None) -> np.ndarray:
    """One launch of entry `name` over (n, in_words) records of 32-bit words; (n, out_words) uint32
    back.  A ladder entry also takes its parameter record (ladder_par)."""
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
    stream = torch.cuda.current_stream().cuda_stream
    if name in LADDERS:
        assert par is not None and par.shape == (PAR_WORDS,) and int(par[4]) >= (n + 255) // 256 * 256
        dpar = torch.from_numpy(np.ascontiguousarray(par, dtype=np.uint32).view(np.int32).copy()).cuda()
        rc = getattr(lib, name)(dpar.data_ptr(), din.data_ptr(), dout.data_ptr(), n, stream)
    else:
        assert par is None
        rc = getattr(lib, name)(din.data_ptr(), dout.data_ptr(), n, stream)
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


def ragged(records: np.ndarray) -> np.ndarray:
    """Records with the first one repeated at the end where the count would fill the last wave."""
    return records if len(records) % 64 else np.concatenate([records, records[:1]])


def to_words(xs, k: int) -> np.ndarray:
    """Python integers -> (N, k) uint32 little-endian words."""
    return np.array([[(int(x) >> (32 * i)) & 0xFFFFFFFF for i in range(k)] for x in xs], dtype=np.uint32).reshape(-1, k)


def words_value(words: np.ndarray):
    """(N, k) little-endian 32-bit words -> list of Python integers."""
    return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in np.asarray(words, dtype=np.uint32)]


def signed(words: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(words).view(np.int32).astype(np.int64)


def run_recode(xs, Ws, W4s) -> np.ndarray:
    """probe_half_recode over (x, W, W4) triples in any order: the records are grouped by (W, W4) and
    each group padded to whole waves (the entry takes W and W4 from a wave's first lane), one launch."""
    groups = {}
    for i, key in enumerate(zip(Ws, W4s)):
        groups.setdefault(key, []).append(i)
    rows, where = [], np.empty(len(xs), dtype=np.int64)
    for (W, W4), idx in sorted(groups.items()):
        for j, i in enumerate(idx):
            where[i] = len(rows) + j
        padded = idx + [idx[0]] * (-len(idx) % 64)
        rows += [[(int(xs[i]) >> (32 * k)) & 0xFFFFFFFF for k in range(5)] + [W, W4] for i in padded]
    rec = np.array(rows, dtype=np.uint32)
    assert all(len({tuple(r) for r in rec[a:a + 64, 5:].tolist()}) == 1 for a in range(0, len(rec), 64))
    return run("probe_half_recode", rec)[where]


def ladder_par(scratch, slots: int, base24, key_tables=None, keys: int = 0) -> np.ndarray:
    """The ladder entries' parameter record: base24 (a prim_probe.Table of 2 x (2^23 + 1) padded
    entries), a test-owned scratch tensor of SLOT_BYTES per lane slot, and the committee's key tables."""
    assert base24.stride == 128 and base24.elements == 2 * ((1 << 23) + 1)
    assert scratch.is_cuda and scratch.numel() * scratch.element_size() >= slots * SLOT_BYTES and slots % 256 == 0
    assert scratch.data_ptr() % 16 == 0
    kt = 0
    if key_tables is not None:
        assert key_tables.stride == 120 and key_tables.elements == 129 * keys and keys > 0
        kt = key_tables.address
    a, s = base24.address, scratch.data_ptr()
    return np.array([a & 0xFFFFFFFF, a >> 32, s & 0xFFFFFFFF, s >> 32, slots, kt & 0xFFFFFFFF, kt >> 32, keys],
                    dtype=np.uint32)
