"""The non-negative field of the half-size verify path (narwhal_amd/csrc/fe_u25519.h, ge_u25519.h) on the CPU.

tests/cpp/feu_host.cpp is a stand-alone program around the host build of the headers (plain u64
arithmetic where the device uses v_mad_u64_u32), built with the address and undefined-behaviour
sanitizers linked into the program itself and run as a child process.  Checked here:
  * every field operation and both conversions against Python integers on ~100k operand pairs;
  * for every (left class, right class) pair of a call site, the product evaluated at the classes'
    maxima with 64-bit operands and 128-bit columns: no prepared operand reaches 2^32, no column
    2^64, and the result is tight.  Limbs are non-negative, so the maxima are the worst case.
    A new call site with a new pair of classes has to be added to MUL_SITES / SQ_SITES / SUB_SITES;
  * the doubling and the table / Niels additions against oracle/ed25519_ref.py.
The device build of the same operations (feu_asm.h's v_mad_u64_u32 half) is held to the same operand rows,
limb for limb against this host build, by tests/test_gpu_prims.py::test_unsigned_field_on_the_device.
"""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests.conftest import ROOT

P = 2**255 - 19
OFFS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
WID = [26, 25] * 5
P_LIMBS = [(P >> o) & ((1 << w) - 1) for o, w in zip(OFFS, WID)]
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
CSRC = os.path.join(ROOT, "narwhal_amd", "csrc")

# ---- operand classes: per-limb maxima (fe_u25519.h's bound contract) --------------------------
TIGHT = [(1 << w) - 1 + (1 << 11) for w in WID]
TIGHT[1] = (1 << 25) - 1 + (1 << 18)
SIGNED_TIGHT = [int(1.01 * 2 ** (w - 1)) for w in WID]   # fe25519.h: |f_i| <= 1.01 * 2^25 / 2^24


def times(k):
    return [int(k * t) for t in TIGHT]


NIELS_SUM = [2 * p + 2 * s for p, s in zip(P_LIMBS, SIGNED_TIGHT)]   # (y + x) + 2p of a signed table entry
NIELS_T = [p + s for p, s in zip(P_LIMBS, SIGNED_TIGHT)]             # 2dxy + p
CLASSES = {"T": TIGHT, "2T": times(2), "3T": times(3), "4T": times(4), "5T": times(5), "3.3T": times(3.3),
           "9.5T": times(9.5), "2p": [2 * p for p in P_LIMBS], "N3": NIELS_SUM, "N1": NIELS_T}

# (left, right) of every feu_mul call site (ge_u25519.h, kernels.hip), then the contract's own limits
MUL_SITES = [
    ("5T", "3T"), ("4T", "3T"),                 # geu_p1p1_to_p2 / _to_p3: X.T, X.Y; Z.Y, Z.T
    ("2T", "3T"), ("3T", "3T"), ("T", "3T"),    # geu_add_cached: pp, mm, zz2 and tt
    ("2T", "N3"), ("3T", "N3"), ("T", "N1"),    # geu_add_niels: pp, mm, tt
    ("2T", "T"),                                # geu_p3_to_cached: T.2d;  geu_decompress: x.y
    ("T", "T"), ("3T", "T"),                    # geu_decompress: the chain; u.v7, u.v3, u.sqrt(-1)
    ("9.5T", "3.3T"), ("5T", "3T"), ("3T", "3T"),
]
SQ_SITES = ["T", "2T", "3T", "3.3T"]            # the chains and Y, Z; a decoded X; X + Y; the contract
SQ2_SITES = ["T", "3.3T"]
# (K, subtrahend class) of every feu_sub<K> / feu_neg<K>
SUB_SITES = [(2, "T"), (3, "2T"), (4, "3T"), (2, "2p")]


def limbs_of(x):
    return [(x >> o) & ((1 << w) - 1) for o, w in zip(OFFS, WID)]


def raw_limbs(x):
    """limbs of x < 2^255 as decoded from bytes (no reduction)."""
    assert 0 <= x < 1 << 255
    return limbs_of(x)


def values(arr):
    """(N, 10) limbs -> object array of Python integers."""
    acc = np.zeros(arr.shape[0], dtype=object)
    for i in range(10):
        acc = acc + (arr[:, i].astype(object) << OFFS[i])
    return acc


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "feu_host_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    "-o", out, os.path.join(ROOT, "tests", "cpp", "feu_host.cpp")], check=True)
    return out


def run(exe, args, **kw):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def field_operands():
    """Rows of (a, b) and their tags: 'T' rows are valid for every operation, 'L:R' rows for the product of that pair."""
    rng = random.Random(25519)
    nrng = np.random.default_rng(25519)
    rows, tags = [], []

    def add(a, b, tag):
        rows.append(list(a) + list(b))
        tags.append(tag)

    ones = [(1 << w) - 1 for w in WID]
    for _ in range(40000):                                      # uniform values, canonical limbs
        add(limbs_of(rng.randrange(P)), limbs_of(rng.randrange(P)), "T")
    for i in range(19 * 19):                                    # every pair of values in [p, 2^255)
        add(raw_limbs(P + i // 19), raw_limbs(P + i % 19), "T")
    for _ in range(5000):                                       # [p, 2^255) against uniform values
        add(raw_limbs(P + rng.randrange(19)), limbs_of(rng.randrange(P)), "T")
        add(limbs_of(rng.randrange(P)), raw_limbs(P + rng.randrange(19)), "T")
    add(ones, ones, "T")
    add(ones, limbs_of(rng.randrange(P)), "T")
    add(limbs_of(rng.randrange(P)), ones, "T")
    add(TIGHT, TIGHT, "T")
    a = np.array(rows, dtype=np.uint32)
    parts, ptags = [a], list(tags)
    for left, right in sorted(set(MUL_SITES)):                  # each pair: the maxima, then random loose limbs
        lm, rm = np.array(CLASSES[left], dtype=np.int64), np.array(CLASSES[right], dtype=np.int64)
        n = 3500
        blk = np.concatenate([nrng.integers(0, lm + 1, size=(n, 10)), nrng.integers(0, rm + 1, size=(n, 10))], axis=1)
        blk[0, :10], blk[0, 10:] = lm, rm
        blk[1, :10] = lm                                        # maxima against random, both ways
        blk[2, 10:] = rm
        parts.append(blk.astype(np.uint32))
        ptags += ["%s:%s" % (left, right)] * n
    return np.concatenate(parts), ptags


def test_field_ops_against_integers(exe, tmp_path):
    ops, tags = field_operands()
    assert len(ops) >= 90000
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    ops.tofile(fin)
    run(exe, ["field", fin, fout])
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(ops), 11, 10)
    check_field_output(ops, tags, out)


def check_field_output(ops, tags, out):
    """The `field` records (feu_host.cpp's layout, 11 x 10 words per operand pair) against integers:
    values mod p and the tightness of every product.  tests/test_gpu_prims.py applies the same checks to
    the device build of the same operations."""
    a, b = values(ops[:, :10]), values(ops[:, 10:])
    tags = np.array(tags)
    tight = np.array(TIGHT, dtype=np.int64)
    bmax = ops[:, 10:].astype(np.int64)

    def check(k, expect, rows, want_tight):
        got = values(out[rows, k, :])
        bad = np.nonzero((got - expect[rows]) % P != 0)[0]
        assert bad.size == 0, (k, rows[bad[:3]], tags[rows[bad[:3]]])
        if want_tight:
            over = np.nonzero((out[rows, k, :].astype(np.int64) > tight).any(axis=1))[0]
            assert over.size == 0, (k, rows[over[:3]], tags[rows[over[:3]]])

    everyone = np.arange(len(ops))
    check(0, a * b, everyone, True)                                                  # feu_mul
    sq_ok = np.nonzero((bmax <= np.array(CLASSES["3.3T"], dtype=np.int64)).all(axis=1))[0]
    assert sq_ok.size > 60000
    check(1, b * b, sq_ok, True)                                                     # feu_sq
    check(2, 2 * b * b, sq_ok, True)                                                 # feu_sq2
    check(3, a + b, everyone, False)                                                 # feu_add
    for k, K in ((4, 2), (5, 3), (6, 4)):                                            # feu_sub<K>: b <= K p limb by limb
        rows = np.nonzero((bmax <= K * np.array(P_LIMBS, dtype=np.int64)).all(axis=1))[0]
        assert rows.size > 45000
        check(k, a - b, rows, False)
        assert (out[rows, k, :].astype(np.int64) <= ops[rows, :10].astype(np.int64) + K * np.array(P_LIMBS)).all()
    check(7, a, everyone, False)                                                     # feu_weak: value kept,
    weak_slack = np.array([(1 << w) - 1 + 19 * 64 for w in WID], dtype=np.int64)    # limbs back to mask + carry
    assert (out[:, 7, :].astype(np.int64) <= weak_slack).all()
    # conversions: s_i = b_i - 2^(w_i - 1) is a signed element; + K p is its non-negative form
    s = values((ops[:, 10:] & 0x7FFFFFFF).astype(np.uint32)) - sum(1 << (o + w - 1) for o, w in zip(OFFS, WID))
    conv = np.nonzero((bmax < 1 << 31).all(axis=1))[0]
    check(8, s, conv, False)
    check(9, s, conv, False)
    t_rows = np.nonzero(tags == "T")[0]                                              # a tight signed element + p: class 2
    assert (out[t_rows, 8, :].astype(np.int64) <= np.array(CLASSES["2T"])).all()
    assert (out[:, 10, :] == ops[:, :10]).all()                                      # to_signed: the same limbs


def test_no_column_or_operand_overflows_at_class_maxima(exe):
    queries = ["mul %s %s" % (" ".join(map(str, CLASSES[l])), " ".join(map(str, CLASSES[r]))) for l, r in MUL_SITES]
    queries += ["sq %s" % " ".join(map(str, CLASSES[c])) for c in SQ_SITES]
    queries += ["sq2 %s" % " ".join(map(str, CLASSES[c])) for c in SQ2_SITES]
    names = ["mul %s x %s" % s for s in MUL_SITES] + ["sq " + c for c in SQ_SITES] + ["sq2 " + c for c in SQ2_SITES]
    lines = run(exe, ["bounds"], input="\n".join(queries) + "\n").strip().splitlines()
    assert len(lines) == len(queries)
    for name, line in zip(names, lines):
        f = [int(x) for x in line.split()]
        op_max, col_max, limbs = f[0], (f[1] << 64) | f[2], f[3:]
        # what limb 0's last carry can leave on limb 1: the largest column bounds column 9's carry
        slack = (19 * (col_max >> 25) + (1 << 26)) >> 26
        print("%-18s operand 2^%.2f column 2^%.2f limb 1 slack <= 2^%.2f" % (name, np.log2(max(op_max, 1)), np.log2(float(col_max)),
                                                                          np.log2(slack)))
        assert slack <= 1 << 18, name
        assert op_max < 1 << 32, name
        assert col_max < 1 << 64, name
        assert all(l <= t for l, t in zip(limbs, TIGHT)), (name, limbs)
    # a pair past the contract does overflow: the shadow can tell
    f = [int(x) for x in run(exe, ["bounds"], input="mul %s %s\n" % (" ".join(map(str, times(4))), " ".join(map(str, times(4))))).split()]
    assert f[0] >= 1 << 32
    for K, cls in SUB_SITES:
        assert all(b <= K * p for b, p in zip(CLASSES[cls], P_LIMBS)), (K, cls)


def ext(point, z, flip_x):
    """Extended coordinates (X:Y:Z:T) of an affine point as limbs; flip_x: X and T as 2p - (-X)."""
    x, y = point
    X, Y, T = x * z % P, y * z % P, x * y % P * z % P
    if flip_x:
        xl = [2 * p - l for p, l in zip(P_LIMBS, limbs_of((-X) % P))]
        tl = [2 * p - l for p, l in zip(P_LIMBS, limbs_of((-T) % P))]
    else:
        xl, tl = limbs_of(X), limbs_of(T)
    return xl + limbs_of(Y) + limbs_of(z) + tl


def affine(rec):
    X, Y, Z, T = (sum(int(l) << o for l, o in zip(rec[10 * k:10 * k + 10], OFFS)) % P for k in range(4))
    assert Z != 0
    zi = pow(Z, P - 2, P)
    assert (T * Z - X * Y) % P == 0
    return (X * zi % P, Y * zi % P)


def test_group_formulas_against_the_oracle(exe, tmp_path):
    rng = random.Random(8)
    small = ref.small_order_points()
    assert len(small) == 8
    pts = list(small) + [ref.pt_mul(rng.randrange(1, 1 << 64), ref.BASEPOINT) for _ in range(8)]
    pts += [ref.pt_add(pts[8], small[3]), ref.pt_add(pts[9], small[5])]           # mixed-order points
    identity = (0, 1)
    assert identity in small
    recs, want = [], []
    for i, p in enumerate(pts):
        for j, q in enumerate(pts):
            neg = (i + j) & 1
            z = rng.randrange(1, P)
            recs.append(ext(p, z, (i ^ j) & 2 != 0) + ext(q, 1, j & 1 != 0) + [neg])
            want.append((p, q, neg))
    # encodings with y >= p: the identity as p + 1, the order-4 points as p + 0 (Z = 1, limbs as decoded)
    for p in [s for s in small if s[1] < 19]:
        for q in pts[6:10]:
            rec = ext(p, 1, False)
            rec[10:20] = raw_limbs(P + p[1])
            recs.append(rec + ext(q, 1, False) + [0])
            want.append((p, q, 0))
    fin, fout = str(tmp_path / "g.bin"), str(tmp_path / "g.out")
    np.array(recs, dtype=np.uint32).tofile(fin)
    run(exe, ["group", fin, fout])
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(recs), 5, 40)
    for (p, q, neg), o in zip(want, out):
        assert affine(o[0]) == ref.pt_add(p, p)
        s = ref.pt_add(p, ref.pt_neg(q) if neg else q)
        assert affine(o[1]) == s
        assert affine(o[2]) == s
        assert affine(o[3]) == s
        assert affine(o[4]) == ref.pt_add(ref.pt_neg(p), ref.pt_neg(p))
