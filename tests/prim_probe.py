"""The primitive probe (tests/hip/prim_probe.hip): its build, its ctypes wrapper, the operand rows and
the checkers of tests/test_gpu_prims.py.

The probe is one shared library around the device-only primitives of narwhal_amd/csrc, compiled
with exactly the library's flags (narwhal_amd.build.FLAGS) into tests/cpp/build/libnwc_probe.so.
It embeds a hash of its source, of every csrc header and of the flags; `load()` refuses a library
whose hash differs from the tree's (a stale or missing probe fails the GPU tests, it does not skip
them), and `build_probe()` rebuilds exactly then.

The checkers are plain functions over numpy arrays and Python integers: they need no device, and
tests/test_prims_host.py feeds each of them a right answer and one wrong answer of every kind.
"""
from __future__ import annotations

import ctypes
import glob
import hashlib
import os
import random
import subprocess

import numpy as np

from oracle import ed25519_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hip", "prim_probe.hip")
OUT = os.path.join(ROOT, "tests", "cpp", "build", "libnwc_probe.so")

P = 2**255 - 19
L = ref.L
OFFS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
WID = [26, 25] * 5

# words per record (in, out) of every entry; probe_record_words() in the library holds the same table
ENTRIES = {
    "probe_fe_ops": (21, 40), "probe_fe_words": (8, 28), "probe_fe_canon": (20, 11), "probe_fe_pow": (10, 20),
    "probe_fes_ops": (21, 80), "probe_fes_pow": (10, 16), "probe_gs": (80, 324), "probe_feu_field": (20, 110),
    "probe_sc_reduce": (16, 8), "probe_sc_lt_l": (8, 1), "probe_sc_recode": (8, 104),
    "probe_decompress1": (8, 50), "probe_decompress2": (16, 100), "probe_geu_decompress": (8, 50),
    "probe_ge_ops": (110, 340), "probe_table_gather": (4, 32),
    "probe_table_audit": (9, 1),   # one parameter record per launch, one flag word per entry (audit_table)
}
# records one 256-lane block holds: a lane, a 16-lane row or a wave per record
PER_BLOCK = {name: 256 for name in ENTRIES}
PER_BLOCK.update({"probe_fes_ops": 16, "probe_fes_pow": 16, "probe_gs": 4})
# (BITS, WINDOWS) of the generic recoding: its radix-4096 wrapper, the basepoint comb, the key comb
RECODE_SHAPES = [(12, 22), (22, 12), (14, 19)]


# ---- build ------------------------------------------------------------------------------------
def probe_sources():
    from narwhal_amd import build as nb
    return [SRC] + sorted(glob.glob(os.path.join(nb.CSRC, "*.h")))


def probe_source_id() -> str:
    from narwhal_amd import build as nb
    h = hashlib.sha256(" ".join(f for f in nb.FLAGS if not f.startswith("-I")).encode())
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
    i = blob.find(b"NWC_PROBE_ID:")
    if i < 0:
        return None
    return blob[i + 13:blob.find(b"\0", i)].decode(errors="replace")


def probe_up_to_date(path: str = OUT) -> bool:
    return embedded_probe_id(path) == probe_source_id()


def build_probe(out: str = OUT, force: bool = False) -> str:
    """hipcc with the library's own flags; rebuilt when the probe source, a csrc header or a flag changed."""
    from narwhal_amd import build as nb
    if out == OUT:   # the in-tree build (__graft_entry__.build()) carries the half-size probe with it
        from tests import half_probe
        half_probe.build_probe(force=force)
    if not force and probe_up_to_date(out):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [nb.HIPCC] + nb.FLAGS + ['-DNWC_PROBE_ID="%s"' % probe_source_id(), "-o", out + ".tmp", SRC]
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
    assert name != "probe_table_audit", "one parameter record per launch: use audit_table()"
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
    return out[:n].copy()


def run_whole_and_ragged(name: str, records: np.ndarray, counts) -> np.ndarray:
    """The whole record set in one launch (more than one block, a ragged last wave -- for the sliced
    probes idle rows / waves in the last block), then the first n records alone for every n in
    `counts`: a short launch must give the same words as the whole one.  Returns the whole output."""
    n = len(records)
    per = PER_BLOCK[name]
    assert n > per, (name, n)
    assert n % (64 if per == 256 else 4) != 0, (name, n)
    whole = run(name, records)
    for c in counts:
        part = run(name, records[:c])
        assert (part == whole[:c]).all(), "%s: a launch of %d records differs from the whole launch" % (name, c)
    return whole


def ragged(records: np.ndarray, name: str) -> np.ndarray:
    """Records with the first one repeated at the end where the count would fill the last wave / block."""
    unit = 64 if PER_BLOCK[name] == 256 else 4
    return records if len(records) % unit else np.concatenate([records, records[:1]])


# ---- stored tables ----------------------------------------------------------------------------
AUDIT_CHAIN, AUDIT_NIELS, AUDIT_BOUND, AUDIT_PAD = 1, 2, 4, 8


class Table:
    """A table of affine Niels entries in device memory: `elements` entries of `stride` bytes (120, or
    128 with two pad words) at `address`.  The probe reads what it is told to, so every reader below
    checks its indices against `elements` first; `owner` keeps a test-owned tensor alive."""

    def __init__(self, address: int, stride: int, elements: int, owner=None):
        assert stride in (120, 128) and address % 4 == 0 and elements >= 0
        self.address, self.stride, self.elements, self.owner = int(address), int(stride), int(elements), owner

    def part(self, first: int, count: int) -> "Table":
        assert 0 <= first and first + count <= self.elements
        return Table(self.address + first * self.stride, self.stride, count, self.owner)


def library_table(name: str):
    """nwc_diag_table of the calling thread's device: (Table or None if not built, keys held)."""
    from narwhal_amd import _lib
    lib = _lib.load()
    addr, elem, count, keys = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
    _lib.check(lib.nwc_diag_table(name.encode(), ctypes.byref(addr), ctypes.byref(elem), ctypes.byref(count),
                                  ctypes.byref(keys)))
    if addr.value == 0:
        assert count.value == 0 and keys.value == 0, name
        return None, 0
    if elem.value in (120, 128):
        return Table(addr.value, elem.value, count.value), keys.value
    return (addr.value, elem.value, count.value), keys.value


def read_array(array) -> np.ndarray:
    """A key or flag array of library_table() -- (address, element bytes, elements) with 32-byte keys
    or 4-byte flag words -- through the gather entry: (elements, element bytes / 4) uint32 words."""
    address, elem, count = array
    assert elem in (4, 32) and address % 4 == 0 and count > 0
    rec = np.empty((count, 4), dtype=np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = address & 0xFFFFFFFF, address >> 32, elem, np.arange(count)
    return run("probe_table_gather", rec)[:, :elem // 4]


def gather(table: Table, indices) -> np.ndarray:
    """Entries `indices` of a table: (n, 32) uint32 words (30 limbs, then the pad words or zeros)."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    assert idx.size and (idx >= 0).all() and (idx < table.elements).all(), "index outside the table"
    rec = np.empty((idx.size, 4), dtype=np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = table.address & 0xFFFFFFFF, table.address >> 32, table.stride, idx
    return run("probe_table_gather", rec)


def audit_table(table: Table, windows: int, entries: int, one_offset: int = 1, one_stride: int = None):
    """probe_table_audit over windows x entries entries: (indices, flag words) of the flagged entries."""
    import torch
    lib = load()
    one_stride = entries if one_stride is None else one_stride
    n = windows * entries
    assert 0 < n <= table.elements and n < 1 << 32 and entries >= 2
    assert 0 <= one_offset and one_offset + (windows - 1) * one_stride < table.elements
    par = np.array([table.address & 0xFFFFFFFF, table.address >> 32, table.stride, windows, entries, one_offset,
                    one_stride, int(TIGHT[0]), int(TIGHT[1])], dtype=np.uint32)
    din = torch.from_numpy(par.view(np.int32).copy()).cuda()
    dout = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = lib.probe_table_audit(din.data_ptr(), dout.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(dout[n]) == 0x5A5A5A5A, "probe_table_audit wrote past its last entry"
    bad = torch.nonzero(dout[:n]).reshape(-1)
    return bad.cpu().numpy().astype(np.int64), dout[:n][bad].cpu().numpy().view(np.uint32)


def device_copy(words: np.ndarray) -> Table:
    """A test-owned device copy of (n, 32) entry words as a table of 128-byte entries."""
    import torch
    words = np.ascontiguousarray(words, dtype=np.uint32)
    assert words.ndim == 2 and words.shape[1] == 32
    t = torch.from_numpy(words.view(np.int32).copy()).cuda()
    return Table(t.data_ptr(), 128, len(words), owner=t)


LANE_COUNTS = (1, 63, 64, 65, 257)
ROW_COUNTS = (1, 2, 3, 4, 5, 7)

# ---- limbs and classes ------------------------------------------------------------------------
TIGHT = np.array([int(1.01 * 2 ** (w - 1)) for w in WID], dtype=np.int64)    # fe25519.h "tight"
LOOSE = np.array([int(1.65 * 2 ** w) for w in WID], dtype=np.int64)          # fe25519.h "loose"
RAW = np.array([(1 << w) - 1 for w in WID], dtype=np.int64)                  # fe_from_words limbs
# fes_mul_small's own output bound (fe_sliced.h): centred limbs + a carry below 2^18, x 19 into limb 0
FES_SMALL_OUT = np.array([(1 << (w - 1)) + (1 << 18) for w in WID], dtype=np.int64)
FES_SMALL_OUT[0] = (1 << 25) + 19 * (1 << 18)
SIGNED_CLASSES = {"T": TIGHT, "2T": 2 * TIGHT, "3T": 3 * TIGHT, "L": LOOSE, "RAW": RAW,
                  "G": TIGHT + FES_SMALL_OUT}                                # t1 + 121666 e (gs_xonly_dbl_n)
# the unsigned field's classes (fe_u25519.h), as tests/test_feu_host.py writes them
FEU_TIGHT = np.array([(1 << w) - 1 + (1 << 11) for w in WID], dtype=np.int64)
FEU_TIGHT[1] = (1 << 25) - 1 + (1 << 18)


def limbs_of(x: int):
    """Limbs of 0 <= x < 2^255 as decoded from bytes."""
    return [(x >> o) & ((1 << w) - 1) for o, w in zip(OFFS, WID)]


def centred_limbs(x: int):
    """x mod p as signed limbs in [-2^(w-1), 2^(w-1)) (+19 on limb 0 at most): tight."""
    x %= P
    out, c = [], 0
    for o, w in zip(OFFS, WID):
        v = ((x >> o) & ((1 << w) - 1)) + c
        c = (v + (1 << (w - 1))) >> w
        out.append(v - (c << w))
    out[0] += 19 * c
    return out


def values(limbs: np.ndarray) -> np.ndarray:
    """(N, 10) signed limbs -> object array of Python integers."""
    acc = np.zeros(limbs.shape[0], dtype=object)
    for i in range(10):
        acc = acc + (limbs[:, i].astype(np.int64).astype(object) << OFFS[i])
    return acc


def signed(words: np.ndarray) -> np.ndarray:
    """uint32 words as signed limbs (int64)."""
    return np.ascontiguousarray(words).view(np.int32).astype(np.int64)


def words_value(words: np.ndarray) -> np.ndarray:
    """(N, k) little-endian 32-bit words -> object array of Python integers."""
    acc = np.zeros(words.shape[0], dtype=object)
    for i in range(words.shape[1]):
        acc = acc + (words[:, i].astype(np.uint64).astype(object) << (32 * i))
    return acc


def to_words(xs, k: int) -> np.ndarray:
    """Python integers -> (N, k) uint32 little-endian words."""
    return np.array([[(int(x) >> (32 * i)) & 0xFFFFFFFF for i in range(k)] for x in xs], dtype=np.uint32)


# ---- checkers ---------------------------------------------------------------------------------
def _first(bad):
    return [int(i) for i in np.nonzero(bad)[0][:4]]


def check_field(limbs: np.ndarray, expect, bound=None, what: str = "") -> None:
    """Signed limbs (N, 10): the value is `expect` mod p and, with a bound, every |limb| is within it."""
    limbs = np.asarray(limbs, dtype=np.int64)
    assert limbs.shape == (len(expect), 10), (what, limbs.shape)
    bad = (values(limbs) - np.asarray(expect, dtype=object)) % P != 0
    assert not bad.any(), "%s: wrong value at rows %s" % (what, _first(bad))
    if bound is not None:
        over = (np.abs(limbs) > np.asarray(bound, dtype=np.int64)).any(axis=1)
        assert not over.any(), "%s: limb out of bound at rows %s: %s" % (what, _first(over), limbs[over][:2].tolist())


def check_unsigned_field(words: np.ndarray, expect, bound, what: str = "") -> None:
    """The same for the non-negative limbs of fe_u25519.h."""
    limbs = np.asarray(words).astype(np.int64)
    check_field(limbs, expect, None, what)
    over = (limbs > np.asarray(bound, dtype=np.int64)).any(axis=1)
    assert not over.any(), "%s: limb out of bound at rows %s" % (what, _first(over))


def check_sliced(lanes: np.ndarray, expect, bound=None, what: str = "") -> None:
    """A sliced element's 16 lanes (N, 16): lanes 10..15 hold zero, lanes 0..9 are check_field's limbs."""
    lanes = np.asarray(lanes, dtype=np.int64)
    assert lanes.shape[1] == 16
    idle = (lanes[:, 10:] != 0).any(axis=1)
    assert not idle.any(), "%s: lanes 10-15 not zero at rows %s" % (what, _first(idle))
    check_field(lanes[:, :10], expect, bound, what)


def check_canonical(words: np.ndarray, expect, modulus: int = P, what: str = "") -> None:
    """(N, 8) words: bit for bit the canonical residue of `expect` (a right value in a
    non-canonical encoding fails)."""
    got = words_value(np.asarray(words, dtype=np.uint32))
    want = np.array([int(e) % modulus for e in expect], dtype=object)
    bad = got != want
    assert not bad.any(), "%s: not the canonical value at rows %s" % (what, _first(bad))


def check_flags(got: np.ndarray, expect, what: str = "") -> None:
    got = np.asarray(got).astype(np.int64).reshape(-1)
    want = np.array([1 if e else 0 for e in expect], dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: flag differs at rows %s" % (what, _first(bad))


def unpack_digits(packed: np.ndarray, bits: int, windows: int) -> np.ndarray:
    """Signed digits of a packed string (N, k words): field w at bits [bits w, bits w + bits), value d + 2^(bits-1)."""
    big = words_value(np.asarray(packed, dtype=np.uint32))
    out = np.zeros((len(big), windows), dtype=np.int64)
    for w in range(windows):
        out[:, w] = np.array([(int(b) >> (bits * w)) & ((1 << bits) - 1) for b in big], dtype=np.int64) - (1 << (bits - 1))
    return out


def check_digits(digits: np.ndarray, bits: int, scalars, what: str = "") -> None:
    """Signed digits (N, windows): each in [-2^(bits-1), 2^(bits-1)), and sum d_i 2^(bits i) = s."""
    digits = np.asarray(digits, dtype=np.int64)
    half = 1 << (bits - 1)
    out = ((digits < -half) | (digits >= half)).any(axis=1)
    assert not out.any(), "%s: digit out of range at rows %s" % (what, _first(out))
    acc = np.zeros(len(digits), dtype=object)
    for i in range(digits.shape[1]):
        acc = acc + (digits[:, i].astype(object) << (bits * i))
    bad = acc != np.array([int(s) for s in scalars], dtype=object)
    assert not bad.any(), "%s: digits do not sum to the scalar at rows %s" % (what, _first(bad))


def point_of(rec: np.ndarray):
    """An extended point's 40 signed limbs -> (X, Y, Z, T) mod p."""
    v = values(np.asarray(rec, dtype=np.int64).reshape(4, 10))
    return tuple(int(x) % P for x in v)


def check_points(recs: np.ndarray, expect, bounds=None, what: str = "") -> None:
    """Extended points (N, 40 signed limbs) against affine points: Z != 0, X/Z and Y/Z equal, T Z = X Y,
    and the limbs of (X, Y, Z, T) within `bounds` (four per-limb maxima)."""
    recs = np.asarray(recs, dtype=np.int64)
    assert len(recs) == len(expect), (what, len(recs), len(expect))
    for i, (rec, want) in enumerate(zip(recs, expect)):
        X, Y, Z, T = point_of(rec)
        assert Z != 0, "%s: Z = 0 at row %d" % (what, i)
        zi = pow(Z, P - 2, P)
        assert (X * zi % P, Y * zi % P) == (want[0] % P, want[1] % P), "%s: wrong point at row %d" % (what, i)
        assert (T * Z - X * Y) % P == 0, "%s: T Z != X Y at row %d" % (what, i)
    if bounds is not None:
        for k, b in enumerate(bounds):
            limbs = recs[:, 10 * k:10 * k + 10]
            over = ((limbs > np.asarray(b)) | (limbs < -np.asarray(b))).any(axis=1)
            assert not over.any(), "%s: coordinate %d out of bound at rows %s" % (what, k, _first(over))


def check_p2(recs: np.ndarray, expect, bounds=None, what: str = "") -> None:
    """Projective points (N, 30 signed limbs: X Y Z) against affine points, as check_points without T."""
    recs = np.asarray(recs, dtype=np.int64)
    assert recs.shape == (len(expect), 30), (what, recs.shape)
    for i, (rec, want) in enumerate(zip(recs, expect)):
        X, Y, Z = (int(x) % P for x in values(rec.reshape(3, 10)))
        assert Z != 0, "%s: Z = 0 at row %d" % (what, i)
        zi = pow(Z, P - 2, P)
        assert (X * zi % P, Y * zi % P) == (want[0] % P, want[1] % P), "%s: wrong point at row %d" % (what, i)
    if bounds is not None:
        for k, b in enumerate(bounds):
            over = (np.abs(recs[:, 10 * k:10 * k + 10]) > np.asarray(b)).any(axis=1)
            assert not over.any(), "%s: coordinate %d out of bound at rows %s" % (what, k, _first(over))


def niels_limbs(point, form: int, rng) -> list:
    """The affine Niels form (ypx, ymx, xy2d) of a point as 30 signed limbs, in the classes a table entry
    comes in: form 0 as ge_p3_to_niels and the comb builders store it (ypx, ymx the limb-wise sum and
    difference of the tight limbs of y and x: up to 2 x tight), form 1 carried (every element tight,
    a packed entry), form 2 with ypx and ymx at the edge of 2 x tight (a tight element with every
    limb at +- its maximum, plus the tight remainder).  xy2d is tight in every form."""
    x, y = point
    cx, cy = np.array(centred_limbs(x)), np.array(centred_limbs(y))
    if form == 0:
        ypx, ymx = cy + cx, cy - cx
    elif form == 1:
        ypx, ymx = np.array(centred_limbs(y + x)), np.array(centred_limbs(y - x))
    else:
        out = []
        for v in (y + x, y - x):
            a = TIGHT * np.array([rng.choice((-1, 1)) for _ in range(10)])
            out.append(a + np.array(centred_limbs(v - int(values(a[None, :])[0]))))
        ypx, ymx = out
    return [int(v) for v in np.concatenate([ypx, ymx, centred_limbs(2 * ref.D * x * y)])]


DECODE_TIGHT = (TIGHT, TIGHT, TIGHT, TIGHT)                    # ge_decompress*: every coordinate tight
DECODE_FEU = (2 * FEU_TIGHT, FEU_TIGHT, FEU_TIGHT, FEU_TIGHT)  # geu_decompress: X <= 2 T, the rest T


def decode_reference(encodings: np.ndarray):
    """(N, 8) words -> [(point or None, y mod p, small-order flag)] by oracle/ed25519_ref.py."""
    small_y = {pt[1] for pt in ref.small_order_points()}
    out = []
    for w in np.asarray(encodings, dtype=np.uint32):
        b = w.astype("<u4").tobytes()
        y = (int.from_bytes(b, "little") & ((1 << 255) - 1)) % P
        out.append((ref.decompress(b), y, y in small_y))
    return out


def check_decode(out: np.ndarray, reference, bounds, nonneg: bool = False, what: str = "") -> None:
    """A decoding probe's 50-word records (X Y Z T, ok, canonical y, small-order flag) against
    decode_reference(): the flags agree, y is canonical, and where ok holds the point is the
    oracle's, T Z = X Y and the limbs are inside `bounds` (nonneg: limbs are unsigned)."""
    out = np.asarray(out, dtype=np.uint32)
    assert out.shape == (len(reference), 50), (what, out.shape)
    check_flags(out[:, 40], [r[0] is not None for r in reference], what + " ok")
    check_canonical(out[:, 41:49], [r[1] for r in reference], P, what + " canonical y")
    check_flags(out[:, 49], [r[2] for r in reference], what + " small order")
    rows = [i for i, r in enumerate(reference) if r[0] is not None]
    limbs = out[rows, :40].astype(np.int64) if nonneg else signed(out[rows, :40])
    if nonneg:
        assert (out[rows, :40] < (1 << 31)).all(), what
    check_points(limbs, [reference[i][0] for i in rows], bounds, what)


# ---- operand rows -----------------------------------------------------------------------------
# (left class, right class) of every fe_mul in ge25519.h and every fes_mul in ge_sliced.h; a completed
# point's coordinates are X 3T, Y 2T, Z 3T, T 3T at most (ge_p2_dbl: E = a - (yy + xx), -F = b - G;
# the additions: 2 zz +- tt), a decoded y is RAW until it is tightened.
FE_MUL_SITES = [
    ("3T", "3T"),                 # ge_p1p1_to_p2 / _to_p3 (and _acc): X.T, Z.T
    ("2T", "3T"),                 # ge_p1p1_to_p2 / _to_p3: Y.Z
    ("3T", "2T"),                 # X.Y;  _acc: Z.Y (19 Y fits for a sum of two tight elements)
    ("T", "T"),                   # ge_p3_to_cached T.2d; ge_add_cached tt, zz; ge_add_niels tt; decompression's products
    ("2T", "2T"),                 # ge_add_cached / ge_add_niels: (Y + X) q.YpX, (Y - X) q.YmX (a table entry is a sum of two tight)
    ("2T", "T"),                  # the same against a carried (packed) table entry
]
FE_SQ_SITES = ["T", "2T", "RAW"]  # ge_p2_dbl: X, Y; X + Y; ge_decompress_prep / _finish: y as decoded
FE_SQ2_SITES = ["T"]              # ge_p2_dbl: 2 Z^2
FES_MUL_SITES = [
    ("T", "T"),                   # gs_dbl X.X, Y.Y; gs_add_cached T.T2d, Z.Z; gs_to_cached T.2d; gs_from_affine X.Y; x-only t0.t1
    ("T", "2T"),                  # gs_dbl: Z.(2 Z)
    ("2T", "2T"),                 # gs_dbl (X + Y)^2; gs_add_cached (Y + X) q.YpX, (Y - X) q.YmX; x-only (U + W)^2, (U - W)^2
    ("3T", "3T"),                 # gs_to_p2 / gs_to_p3: X.T, Z.T
    ("2T", "3T"),                 # Y.Z
    ("3T", "2T"),                 # X.Y
    ("2T", "G"),                  # gs_xonly_dbl_n: e.(t1 + 121666 e)
]
CONTRACT_PAIRS = [("T", "T"), ("L", "T"), ("T", "L"), ("L", "L")]


def _sign_patterns(nrng, n_random):
    pats = [np.ones(20, dtype=np.int64), -np.ones(20, dtype=np.int64),
            np.array([1, -1] * 10, dtype=np.int64), np.array([-1, 1] * 10, dtype=np.int64),
            np.array([1] * 10 + [-1] * 10, dtype=np.int64), np.array([-1] * 10 + [1] * 10, dtype=np.int64)]
    return np.concatenate([np.array(pats), nrng.integers(0, 2, size=(n_random, 20)) * 2 - 1])


def signed_pair_rows(pairs, seed: int, n_uniform: int = 12000, n_signs: int = 2000, n_mixed: int = 400,
                     n_random: int = 2500):
    """(N, 20) int64 rows (f, g) and a tag per row, for fe_mul / fes_mul and the squarings of f:
      * uniform canonical values as limbs, and the 19 x 19 pairs of values in [p, 2^255) as decoded ("RAW:RAW");
      * for every (left, right) class pair: every limb at +- its maximum (all plus, all minus,
        alternating, halves, n_signs random patterns), maxima against limbs uniform in [-max, max]
        both ways round, and uniform limbs on both sides."""
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    rows = [limbs_of(rng.randrange(P)) + limbs_of(rng.randrange(P)) for _ in range(n_uniform)]
    rows += [limbs_of(P + i // 19) + limbs_of(P + i % 19) for i in range(19 * 19)]
    parts, tags = [np.array(rows, dtype=np.int64)], ["RAW:RAW"] * len(rows)
    for left, right in pairs:
        m = np.concatenate([SIGNED_CLASSES[left], SIGNED_CLASSES[right]])
        pats = _sign_patterns(nrng, n_signs)
        uni = nrng.integers(-m, m + 1, size=(2 * n_mixed + n_random, 20))
        mixed = uni[:2 * n_mixed].copy()
        s = nrng.integers(0, 2, size=(2 * n_mixed, 10)) * 2 - 1
        mixed[:n_mixed, :10] = s[:n_mixed] * m[:10]            # the left operand at its maxima
        mixed[n_mixed:, 10:] = s[n_mixed:] * m[10:]            # the right one
        blk = np.concatenate([pats * m, mixed, uni[2 * n_mixed:]])
        parts.append(blk)
        tags += ["%s:%s" % (left, right)] * len(blk)
    return np.concatenate(parts), np.array(tags)


def small_constants(n: int, limit: int, seed: int) -> np.ndarray:
    """n constants with |c| < limit: the edges first (0, +-1, +-(limit - 1), ...), then uniform."""
    edges = [0, 1, -1, limit - 1, -(limit - 1), 2, -2, limit // 2, -(limit // 2), 19, -19]
    c = np.random.default_rng(seed).integers(-(limit - 1), limit, size=n)
    k = min(n, 40 * len(edges))
    c[:k] = np.resize(np.array(edges, dtype=np.int64), k)
    return c.astype(np.int64)


def word_rows(seed: int, n_uniform: int = 8000) -> np.ndarray:
    """256-bit values for fe_from_words / fe_tighten / fe_to_words: [p, 2^255) with either top bit,
    the edges, every limb at the rounding edges of fe_tighten, uniform strings."""
    rng = random.Random(seed)
    xs = [P + i + (b << 255) for i in range(19) for b in (0, 1)]
    xs += [0, 1, 19, P - 1, P - 2, (1 << 255) - 1, (1 << 256) - 1, 1 << 255, (1 << 255) + 18]
    half = [1 << (w - 1) for w in WID]
    for delta in (-1, 0, 1):                                   # every limb at 2^(w-1) + delta; one limb at a time
        xs.append(sum((h + delta) << o for h, o in zip(half, OFFS)))
        xs += [(h + delta) << o for h, o in zip(half, OFFS)]
        xs += [((1 << 255) - 1) ^ (((1 << w) - 1) << o) | ((h + delta) << o) for h, o, w in zip(half, OFFS, WID)]
    xs += [rng.getrandbits(256) for _ in range(n_uniform)]
    xs += [P - rng.randrange(1 << 20) for _ in range(500)] + [rng.randrange(1 << 40) for _ in range(500)]
    return to_words(xs, 8)


def canon_rows(seed: int, n: int = 66000):
    """Representations of k p + delta, k in 0..3, delta in {0, +-1, 18, 19, 20, -19, -20, random}:
    a (N, 20) int64 array of (a, b) and per row the value of a and of b.  a is rewritten into
    non-canonical limbs by moving a random multiple (up to 3) of 2^w between each pair of neighbouring
    limbs and 19 times that across the top, or built as a sum / difference of three tight elements;
    rows above 7 x tight are dropped, so a - b (fe_equal) stays within the 8 x tight fe_to_words accepts.  b is a tight form
    of the same value, of a neighbour, or of a random value."""
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    deltas = [0, 1, -1, 18, 19, 20, -19, -20]
    vals, base = [], []
    for i in range(n):
        k = i & 3
        d = deltas[(i >> 2) % 9] if (i >> 2) % 9 < 8 else rng.randrange(P)
        v = k * P + d
        vals.append(v)
        if i % 3 == 2:                                          # t1 + t2 - t3, three tight elements
            x1, x2 = rng.randrange(P), rng.randrange(P)
            t = [a + b - c for a, b, c in zip(centred_limbs(x1), centred_limbs(x2), centred_limbs(x1 + x2 - v))]
        elif i % 3 == 1 and v >= 0:                             # the value's own bits; the top limb takes what is past 2^255
            t = limbs_of(v & ((1 << 255) - 1))
            t[9] += (v >> 255) << 25
        else:
            t = centred_limbs(v)
        base.append(t)
    a = np.array(base, dtype=np.int64)
    m = nrng.integers(-3, 4, size=(n, 10))
    m[(np.arange(n) % 3 == 1)[:, None] & (m == -3)] = 3         # limbs as decoded are non-negative: no room for + 3 x 2^w
    m[np.arange(n) % 3 == 2] = 0
    for i in range(10):
        a[:, i] -= m[:, i] << WID[i]
        if i < 9:
            a[:, i + 1] += m[:, i]
        else:
            a[:, 0] += 19 * m[:, i]
    vals = np.array(vals, dtype=object)
    assert ((values(a) - vals) % P == 0).all()
    kind = nrng.integers(0, 4, size=n)                          # b: the same value, +1, -1, a random value
    bvals = [int(v) + (0, 1, -1, 0)[k] if k < 3 else rng.randrange(P) for v, k in zip(vals, kind)]
    b = np.array([centred_limbs(x) for x in bvals], dtype=np.int64)
    keep = (np.abs(a) <= 7 * TIGHT).all(axis=1)
    return np.concatenate([a, b], axis=1)[keep], vals[keep], np.array(bvals, dtype=object)[keep]


def group_points(seed: int = 8):
    """tests/test_feu_host.py's point set: the 8 small-order points, 8 multiples of B, 2 mixed-order points."""
    rng = random.Random(seed)
    small = ref.small_order_points()
    pts = list(small) + [ref.pt_mul(rng.randrange(1, 1 << 64), ref.BASEPOINT) for _ in range(8)]
    pts += [ref.pt_add(pts[8], small[3]), ref.pt_add(pts[9], small[5])]
    return pts


def ext_limbs(point, z: int):
    """(X : Y : Z : T) of an affine point scaled by z, as 40 tight signed limbs."""
    x, y = point
    return centred_limbs(x * z) + centred_limbs(y * z) + centred_limbs(z) + centred_limbs(x * y % P * z)


def ext_limbs_at_maxima(point, which: int, rng):
    """(X : Y : Z : T) of an affine point, 40 tight signed limbs, with coordinate `which` (0 X, 1 Y, 2 Z,
    3 T) at +- the tight maximum in every limb (a random sign pattern): the scale z is chosen so that
    the coordinate has that value, which its limbs then state as they are.  Falls back to Z where the
    point's coordinate is zero (no scale reaches a non-zero value)."""
    x, y = point
    factor = (x, y, 1, x * y % P)[which] % P
    if factor == 0:
        which, factor = 2, 1
    for _ in range(8):
        edge = TIGHT * np.array([rng.choice((-1, 1)) for _ in range(10)])
        z = int(values(edge[None, :])[0]) % P * pow(factor, P - 2, P) % P
        if z:
            break
    out = ext_limbs(point, z)
    assert (int(values(np.array(out[10 * which:10 * which + 10])[None, :])[0]) - int(values(edge[None, :])[0])) % P == 0
    out[10 * which:10 * which + 10] = [int(v) for v in edge]
    return out


def reduce_inputs(seed: int, n_uniform: int = 20000):
    """512-bit inputs of sc_reduce512: the edges, q l - 1 / q l / q l + 1 for small, medium and full-size
    q (where a Barrett estimate is short by one or two), all-ones / all-zero halves, k a + r as
    sign_response forms it, uniform values."""
    rng = random.Random(seed)
    top = (1 << 512) - 1
    xs = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 1 << 252, (1 << 253) - 1, (1 << 256) - 1, 1 << 256,
          (1 << 256) + 1, top, top - 1, top // L * L, top // L * L - 1]
    for bits, count in ((8, 256), (128, 3000), (260, 3000)):
        for i in range(count):
            q = i if bits == 8 else rng.getrandbits(bits)
            xs += [min(max(q * L + d, 0), top) for d in (-1, 0, 1)]
    ones = (1 << 256) - 1
    xs += [ones << 256, ones, (ones << 256) | ones, ((1 << 32) - 1) << 224, ((1 << 288) - 1) << 224, (1 << 224) - 1]
    xs += [sum(0xFFFFFFFF << (32 * i) for i in range(16) if (m >> i) & 1) for m in rng.sample(range(1 << 16), 400)]
    pick = lambda: rng.choice([0, 1, L - 1, rng.randrange(L)])   # noqa: E731
    xs += [pick() * pick() + pick() for _ in range(3000)]
    xs += [(L - 1) * (L - 1) + (L - 1), (L - 1) * (L - 1), (L - 1) + (L - 1)]
    xs += [rng.getrandbits(512) for _ in range(n_uniform)]
    return xs


def lt_l_inputs():
    xs = [0, 1, L - 1, L, L + 1, (1 << 256) - 1, 1 << 252, (1 << 252) - 1, 1 << 253]
    for i in range(8):
        xs += [L + (1 << (32 * i)), L - (1 << (32 * i))]
    return [x for x in xs if 0 <= x < 1 << 256]


def recode_inputs(seed: int, n_uniform: int = 5000):
    """Scalars below 2^253 (the recodings' contract): the edges, every nibble 7 / 8, 7f / 80 bytes,
    7fff / 8000 halfwords, a run of maximal digits ending in each window of each radix, uniform values."""
    rng = random.Random(seed)
    cap = (1 << 253) - 1
    rep = lambda unit, bits: sum(unit << i for i in range(0, 256, bits)) & cap   # noqa: E731
    xs = [0, 1, cap, L - 1, L, 1 << 252, rep(7, 4), rep(8, 4), rep(0x7F, 8), rep(0x80, 8), rep(0x7FFF, 16),
          rep(0x8000, 16), rep(0x78, 8), rep(0x87, 8), rep(0x807F, 16), rep(0x7F80, 16)]
    for bits in (4, 8, 16, 12, 22, 14):
        half = 1 << (bits - 1)
        for w in range(1, 253 // bits + 2):
            for digit in (half - 1, half, (1 << bits) - 1):     # a run of equal digits below window w, and one past it
                run_ = sum(digit << (bits * i) for i in range(w))
                xs += [run_, run_ | (1 << (bits * w)), run_ | (rng.getrandbits(253) << (bits * w))]
    xs += [rng.getrandbits(253) for _ in range(n_uniform)]
    xs += [rng.randrange(L) for _ in range(1000)]
    return [x & cap for x in xs]


def decode_inputs(seed: int, n_points: int = 4000, n_random: int = 4000) -> np.ndarray:
    """Encodings for the decoding probes, (N, 8) words: the small-order points with both sign bits
    (x = 0 with the bit set included), every y in [p, 2^255) and y in {0, 1, p - 1, 2^255 - 1} with
    both bits, multiples of B and mixed-order points, random strings (about half off the curve)."""
    rng = random.Random(seed)
    top = 1 << 255
    xs = []
    for pt in ref.small_order_points():
        e = int.from_bytes(ref.compress(pt), "little")
        xs += [e & (top - 1), e | top]
    for y in list(range(P, top)) + [0, 1, P - 1, top - 1]:
        xs += [y, y | top]
    small = ref.small_order_points()
    pt = ref.pt_mul(rng.randrange(1, L), ref.BASEPOINT)
    step = ref.pt_mul(rng.randrange(1, L), ref.BASEPOINT)
    for i in range(n_points):                                   # a walk: multiples of B, every other one pushed off the prime-order subgroup
        pt = ref.pt_add(pt, step)
        q = ref.pt_add(pt, small[i % 8]) if i & 1 else pt
        xs.append(int.from_bytes(ref.compress(q), "little"))
    xs += [rng.getrandbits(256) for _ in range(n_random)]
    return to_words(xs, 8)
