"""The joint signed radix-4 table of the uncached half-size ladder (narwhal_amd/csrc/ge_u25519.h:
geu_build_joint, geu_recode4, geu_joint_ladder) on the CPU.

tests/cpp/joint_host.cpp is a stand-alone program around the host build of the header, built with the
address and undefined-behaviour sanitizers linked into the program itself and run as a child process.
Checked here:
  * the recoding: sum digit . 4^i is the value, every digit is in {-2..2} (the top one in {0..2}), and the
    joint code 5 a + b names the pair (a, b): |code| is the entry index, its sign the pair's sign;
  * the builder: entry |5 a + b| is a P + b Q against oracle/ed25519_ref.py, every stored coordinate tight
    and every coordinate handed to the pack within its 3 T contract;
  * the bounds: every product, square and subtraction of the new formulas at its classes' maxima in
    128-bit arithmetic (the method of tests/test_feu_host.py, whose classes these are);
  * the ladder without its basepoint term: c P + d Q at forced window counts 66, 67, 70 and 74.
"""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests.conftest import ROOT, GOLDEN
from tests.test_feu_host import (BUILD, CLASSES, CSRC, MUL_SITES, OFFS, P, P_LIMBS, SQ_SITES, SUB_SITES, TIGHT, ext,
                                 limbs_of)

ENTRIES = 13
D2 = 2 * ref.D % P
# entry index -> (a, b): 0 the identity; 5 a + b for a in {1, 2}, b in {-2..2}; b for a = 0
PAIR_OF = {0: (0, 0), 1: (0, 1), 2: (0, 2)}
PAIR_OF.update({5 * a + b: (a, b) for a in (1, 2) for b in range(-2, 3)})
assert sorted(PAIR_OF) == list(range(ENTRIES))

# (left, right) of every feu_mul in geu_dbl_affine / geu_add_affine / geu_build_joint and of the
# operations they call with new operand classes; each must be a pair of the contract (test_feu_host.MUL_SITES)
NEW_MUL_SITES = [
    ("2T", "T"),                  # geu_build_joint: T_P . 2d T_Q;  geu_p3_to_cached of P, Q: T . 2d
    ("3T", "3T"),                 # geu_add_affine: (Y + X)(Y' +- X'), (Y - X)(Y' -+ X')
    ("5T", "3T"), ("4T", "3T"),   # geu_p1p1_to_p3 of geu_dbl_affine (X 4 T, Z 3 T) and of geu_add_affine (X 3 T, Z 3 T)
    ("2T", "3T"), ("T", "T"),     # geu_add_niels with an affine (Y + X, Y - X) <= 3 T and a tight 2d T: pp, tt
]
NEW_SQ_SITES = ["2T", "T"]        # geu_dbl_affine: X, Y
NEW_SUB_SITES = [(2, "2p"), (2, "T")]   # Y - X of a decoded point (X <= 2p limb by limb); 2 - tt, yy - xx


def run(exe, args, **kw):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "joint_host_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    "-o", out, os.path.join(ROOT, "tests", "cpp", "joint_host.cpp")], check=True)
    return out


def words5(x):
    assert 0 <= x < 1 << 160
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(5)]


def min_windows(x):
    """smallest W in [66, 74] with x < 2^(2W - 1)"""
    return max(66, (x.bit_length() + 2) // 2)


# ---- recoding -------------------------------------------------------------------------------------
def recode_values():
    rng = random.Random(4)
    vals = [0, 1, 2, 3]
    for k in range(1, 147):
        vals += [(1 << k) - 1, 1 << k]
    vals.append((1 << 147) - 1)
    # strings that force every carry: all digits 2 (each takes the carry rule's -2 and hands one up), all 3,
    # alternating 2 / 1 (a carry into a 1 makes the next 2), and their shifts
    for n in (64, 65, 66, 70, 73):
        for digit in (2, 3):
            vals.append(sum(digit << (2 * i) for i in range(n)))
        vals.append(sum((2 if i & 1 else 1) << (2 * i) for i in range(n)))
        vals.append(sum((1 if i & 1 else 2) << (2 * i) for i in range(n)))
    vals = [v for v in vals if v < 1 << 147]
    for bits in range(128, 147):
        vals += [rng.getrandbits(bits) | 1 << (bits - 1) for _ in range(40)]
    return vals


def test_recoding_digits_and_joint_code(exe):
    rng = random.Random(5)
    vals = recode_values()
    assert len(vals) > 1000
    rows = []
    for i, c in enumerate(vals):
        d = vals[(7 * i + 3) % len(vals)]
        lo = max(min_windows(c), min_windows(d))
        for W in sorted({lo, min(74, lo + 1), rng.randrange(lo, 75), 74}):
            rows.append((W, c, d))
    text = "\n".join("%d %s %s" % (W, " ".join(map(str, words5(c))), " ".join(map(str, words5(d)))) for W, c, d in rows)
    lines = run(exe, ["recode"], input=text + "\n").strip().splitlines()
    assert len(lines) == len(rows)
    seen = set()
    for (W, c, d), line in zip(rows, lines):
        f = [int(x) for x in line.split()]
        assert len(f) == 3 * W
        a, b, j = f[:W], f[W:2 * W], f[2 * W:]
        for digits, value in ((a, c), (b, d)):
            assert sum(x << (2 * i) if x >= 0 else -((-x) << (2 * i)) for i, x in enumerate(digits)) == value, (W, value)
            assert all(-2 <= x <= 2 for x in digits), (W, value)
            assert all(-2 <= x <= 1 for x in digits[:-1]) and 0 <= digits[-1] <= 2, (W, value)
        for x, y, code in zip(a, b, j):
            assert -12 <= code <= 12
            pa, pb = PAIR_OF[abs(code)]
            assert (x, y) == ((-pa, -pb) if code < 0 else (pa, pb)), (x, y, code)
            seen.add(code)
    # digits below the top are in [-2, 1]: 4 x 4 pairs there, and the top window adds digit 2
    assert {5 * x + y for x in range(-2, 2) for y in range(-2, 2)} <= seen
    assert {5 * x + y for x in range(0, 3) for y in range(0, 3)} <= seen


# ---- the builder ----------------------------------------------------------------------------------
def golden_points():
    """Decoded A and R of every golden verify case: valid keys, small-order and mixed-order points."""
    cases = json.load(open(os.path.join(GOLDEN, "ed25519_verify.json")))["cases"]
    pts = []
    for c in cases:
        for b in (bytes.fromhex(c["pk"]), bytes.fromhex(c["sig"])[:32]):
            p = ref.decompress(b)
            if p is not None and p not in pts:
                pts.append(p)
    return pts


def point_pairs():
    rng = random.Random(9)
    small = ref.small_order_points()
    assert len(small) == 8 and (0, 1) in small
    rnd = [ref.pt_mul(rng.randrange(1, ref.L), ref.BASEPOINT) for _ in range(10)]
    mixed = [ref.pt_add(rnd[0], small[3]), ref.pt_add(rnd[1], small[5]), ref.pt_add(rnd[2], small[7])]
    gold = golden_points()
    assert any(ref.is_small_order(p) for p in gold)
    assert any(ref.has_torsion(p) and not ref.is_small_order(p) for p in gold + mixed)
    pairs = [(rnd[i], rnd[i + 1]) for i in range(0, 10, 2)]
    pairs += [(p, p) for p in rnd[:3] + small + mixed[:1]]                       # P = Q
    pairs += [(p, ref.pt_neg(p)) for p in rnd[:3] + small + mixed[:1]]           # P = -Q
    pairs += [(s, rnd[3]) for s in small] + [(rnd[4], s) for s in small]         # P or Q of small order
    pairs += [(s, t) for s in small[:4] for t in small[4:]]
    pairs += [(m, rnd[5]) for m in mixed] + [(mixed[0], mixed[1]), (rnd[6], mixed[2])]   # mixed order
    pairs += [(gold[i], gold[(5 * i + 1) % len(gold)]) for i in range(len(gold))]
    return pairs


def affine_ext(p, flip):
    """A decoded point: Z = 1, T = x y; flip: X and T as 2p - (-X) (the negated form, class 2 T)."""
    return ext(p, 1, flip)


def value(limbs):
    return sum(int(l) << o for l, o in zip(limbs, OFFS)) % P


def entry_point(rec):
    """(Y+X, Y-X, 2Z, 2dT) as 40 limbs -> the affine point, with 2dT checked against it."""
    ypx, ymx, z2, t2d = (value(rec[10 * k:10 * k + 10]) for k in range(4))
    assert z2 != 0
    zi = pow(z2, P - 2, P)                      # 1 / 2Z
    x, y = (ypx - ymx) * zi % P, (ypx + ymx) * zi % P
    assert (t2d - D2 * x * y % P * z2 * pow(2, P - 2, P)) % P == 0          # T = x y Z
    return (x, y)


def test_builder_entries_against_the_oracle(exe, tmp_path):
    pairs = point_pairs()
    recs = [affine_ext(p, i & 1 != 0) + affine_ext(q, i & 2 != 0) for i, (p, q) in enumerate(pairs)]
    fin, fout = str(tmp_path / "b.bin"), str(tmp_path / "b.out")
    np.array(recs, dtype=np.uint32).tofile(fin)
    run(exe, ["build", fin, fout])
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(recs), ENTRIES * 40 + 1)
    tight = np.array(TIGHT * 4, dtype=np.int64)
    for (p, q), o in zip(pairs, out):
        assert o[-1] == 0                                                   # nothing looser than 3 T reached the pack
        for e in range(ENTRIES):
            a, b = PAIR_OF[e]
            rec = o[40 * e:40 * e + 40]
            assert (rec.astype(np.int64) <= tight).all(), (e, rec)
            assert entry_point(rec) == ref.pt_add(ref.pt_mul(a, p), ref.pt_mul(b, q) if b >= 0 else ref.pt_neg(ref.pt_mul(-b, q))), e


# ---- bounds ---------------------------------------------------------------------------------------
def test_new_sites_hold_at_their_class_maxima(exe):
    assert set(NEW_MUL_SITES) <= set(MUL_SITES)                 # the contract's pairs: held for the device there
    assert set(NEW_SQ_SITES) <= set(SQ_SITES) and set(NEW_SUB_SITES) <= set(SUB_SITES)
    queries = ["mul %s %s" % (" ".join(map(str, CLASSES[l])), " ".join(map(str, CLASSES[r]))) for l, r in NEW_MUL_SITES]
    queries += ["sq %s" % " ".join(map(str, CLASSES[c])) for c in NEW_SQ_SITES]
    lines = run(exe, ["bounds"], input="\n".join(queries) + "\n").strip().splitlines()
    assert len(lines) == len(queries)
    for q, line in zip(queries, lines):
        f = [int(x) for x in line.split()]
        op_max, col_max, limbs = f[0], (f[1] << 64) | f[2], f[3:]
        assert op_max < 1 << 32 and col_max < 1 << 64, q[:8]
        assert ((19 * (col_max >> 25) + (1 << 26)) >> 26) <= 1 << 18           # limb 1's slack
        assert all(l <= t for l, t in zip(limbs, TIGHT)), q[:8]
    for K, cls in NEW_SUB_SITES:
        assert all(b <= K * p for b, p in zip(CLASSES[cls], P_LIMBS)), (K, cls)
    # the sums the new formulas form before a product stay inside the class named at the site
    two_plus_2p = [2 * p + (2 if i == 0 else 0) for i, p in enumerate(P_LIMBS)]    # 2 + 2p - tt, a right operand
    assert all(v <= t for v, t in zip(two_plus_2p, CLASSES["3T"]))
    assert all(2 * v <= t for v, t in zip(CLASSES["2T"], CLASSES["5T"]))           # E = T + T, a left operand
    assert all(t + p2 <= v for t, p2, v in zip(TIGHT, CLASSES["2p"], CLASSES["3T"]))   # Y + 2p - X, Y + X
    assert (1 << 26) - 1 + 2 <= TIGHT[0]                                            # 2 + tt: limb 0 of a product is masked


# ---- the ladder -----------------------------------------------------------------------------------
def test_ladder_without_basepoint_term(exe, tmp_path):
    rng = random.Random(12)
    small = ref.small_order_points()
    pts = [ref.pt_mul(rng.randrange(1, ref.L), ref.BASEPOINT) for _ in range(6)]
    pts += [ref.pt_add(pts[0], small[3]), small[2], small[6]]
    recs, want = [], []
    for W in (66, 67, 70, 74):
        top = 2 * W - 1                                         # scalars below 2^(2W - 1)
        for i in range(80):
            p, q = pts[i % len(pts)], pts[(i * 5 + 1 + i // 9) % len(pts)]
            if i < 60:
                c, d = rng.getrandbits(top), rng.getrandbits(top)
            else:                                               # edge scalars: 0, 1, the largest, short ones
                c = (0, 1, (1 << top) - 1, rng.getrandbits(64))[i & 3]
                d = ((1 << top) - 1, 0, rng.getrandbits(128), 1)[(i >> 2) & 3]
            recs.append(affine_ext(p, i & 1 != 0) + affine_ext(q, i & 2 != 0) + words5(c) + words5(d) + [W])
            want.append(ref.pt_add(ref.pt_mul(c, p), ref.pt_mul(d, q)))
    assert len(recs) >= 300
    fin, fout = str(tmp_path / "l.bin"), str(tmp_path / "l.out")
    np.array(recs, dtype=np.uint32).tofile(fin)
    run(exe, ["ladder", fin, fout])
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(recs), 30)
    tight = np.array(TIGHT * 3, dtype=np.int64)
    for w, o in zip(want, out):
        assert (o.astype(np.int64) <= tight).all()
        X, Y, Z = (value(o[10 * k:10 * k + 10]) for k in range(3))
        assert Z != 0
        zi = pow(Z, P - 2, P)
        assert (X * zi % P, Y * zi % P) == w
