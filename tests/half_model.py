"""Integer models of the half-size scalars and of their digit strings, the record generators and the
checkers of tests/test_gpu_half.py.  No device: tests/test_half_host.py runs the models against each
other and against the host build of lattice.h, and feeds every checker a right answer and one wrong
answer of each kind it claims to catch.

  * euclid(k): the exact remainder sequence of (8l, k) with cofactors, stopped at the first remainder
    below 2^127; model_reduce(k): lat::reduce's choice of (c, d) from its last two rows.
  * check_half_scalars: the four properties the verify kernels rest on (d odd, 0 < d < 2^146,
    |c| < 2^146, d k = c mod 8l), the bit length and the sign flag.
  * digits16 / digits256 / digits24 / digits4: the signed digit strings of kernels.hip and ge_u25519.h.
  * constructed_k: challenges whose reduction ends on an even cofactor with a remainder pair of the
    caller's choice, so max(|c|, d) takes every bit length from 128 past 146.
  * edge rows for the recodings and for base_digits; the ladders' record sets and their checker.
"""
from __future__ import annotations

import math
import random

import numpy as np

from oracle import ed25519_ref as ref

P = 2**255 - 19
L = ref.L
N = 8 * L
HALF_BITS = 146
B24_SPLIT = 141


# ---- lat::reduce ------------------------------------------------------------------------------
def euclid(k: int):
    """Rows (r, t) of Euclid on (8l, k) with t_i k = r_i (mod 8l): the row before the first remainder
    below 2^127, and that row."""
    r0, t0, r1, t1 = N, 0, k, 1
    while r1 >= 1 << 127:
        q = r0 // r1
        r0, t0, r1, t1 = r1, t1, r0 - q * r1, t0 - q * t1
    return (r0, t0), (r1, t1)


def even_branch(rows, m: int):
    (r0, t0), (r1, t1) = rows
    return r0 - m * r1, t0 - m * t1


def model_reduce(k: int):
    """(c, d, ok, m) as lat::reduce forms them: the stopping row when its cofactor is odd (m None), else
    the narrower of (r0 - m r1, t0 - m t1) for m = floor((r0 - |t0|) / (r1 + |t1|)) and m + 1 (the
    kernels estimate that quotient in double precision: a borderline k may land on a neighbour)."""
    rows = euclid(k)
    (r0, t0), (r1, t1) = rows
    if t1 & 1:
        c, d, m = r1, t1, None
    else:
        m0 = min(max((r0 - abs(t0)) // (r1 + abs(t1)), 0), 4294967294)      # the estimate is kept in 32 bits
        best = None
        for m in (m0, m0 + 1):
            c, d = even_branch(rows, m)
            # r0 - m r1 stays non-negative, and |t0| + m |t1| far below the 160 bits of the cofactor words
            if c < 0 or abs(t1).bit_length() + (m | 1).bit_length() > 150:
                continue
            bits = max(c.bit_length(), abs(d).bit_length())
            if best is None or bits < best[0]:
                best = (bits, c, d, m)
        if best is None:
            return 0, 1, False, m0
        _, c, d, m = best
    if d < 0:
        c, d = -c, -d
    ok = max(abs(c).bit_length(), d.bit_length()) <= HALF_BITS
    return c, d, ok, m


def check_half_scalars(k: int, c_abs: int, d: int, c_neg, ok, bits: int, what: str = "") -> None:
    """One device (or host) result against the properties: nothing is asked of (c, d) when ok is clear
    but the bit length and the sign flag, which the kernels read either way."""
    c = -c_abs if c_neg else c_abs
    assert bits == max(c_abs.bit_length(), d.bit_length()), "%s: bits %d of k = %d" % (what, bits, k)
    assert not (c_abs == 0 and c_neg), "%s: c = 0 with the sign set, k = %d" % (what, k)
    if not ok:
        return
    assert d & 1, "%s: d even, k = %d" % (what, k)
    assert 0 < d < 1 << HALF_BITS, "%s: d out of range, k = %d" % (what, k)
    assert c_abs < 1 << HALF_BITS, "%s: c out of range, k = %d" % (what, k)
    assert (d * k - c) % N == 0, "%s: d k != c mod 8l, k = %d" % (what, k)


def check_against_model(k: int, c_abs: int, d: int, c_neg, what: str = "") -> None:
    """Where Euclid stops on an odd cofactor, (c, d) is that row up to the joint sign."""
    (_, _), (r1, t1) = euclid(k)
    if t1 & 1:
        c = -c_abs if c_neg else c_abs
        assert (c, d) == ((r1, t1) if t1 > 0 else (-r1, -t1)), "%s: not Euclid's row, k = %d" % (what, k)


def even_branch_m(k: int, c_abs: int, d: int, c_neg):
    """m with (c, d) = +-(r0 - m r1, t0 - m t1), or None if (c, d) is not of that form."""
    rows = euclid(k)
    (r0, t0), (r1, t1) = rows
    c = -c_abs if c_neg else c_abs
    for sc, sd in ((c, d), (-c, -d)):
        if r1 and (r0 - sc) % r1 == 0:
            m = (r0 - sc) // r1
            if m >= 0 and even_branch(rows, m) == (sc, sd):
                return m
    return None


def ordinary_k():
    """The ordinary set: 20,000 random k, the near-rational k of tests/test_lattice_host.py's
    test_adversarial_structure (the same seed), and the edge list of its test_edge_k."""
    rng = random.Random(5)
    ks = [rng.randrange(L) for _ in range(20000)]
    rng = random.Random(9)
    for _ in range(3000):
        num = rng.randrange(1, 2**20)
        den = rng.randrange(1, 2**20)
        ks.append((N * num // den + rng.randrange(-2**40, 2**40)) % L)
    edge = [0, 1, 2, 3, 5, 2**64, 2**126, 2**127 - 1, 2**127, 2**127 + 1, 2**200, L - 1, L - 2, L // 2, L // 3,
            L // 7, 4 * L // 9, (N - 1) // 2 % L, 2**252, 2**252 + 12345]
    return ks + [k % L for k in edge]


def constructed_k(seed: int, per_size: int = 40):
    """Challenges k < l whose reduction stops on rows (r0, t0), (r1, t1) with t1 even, |t1| of 96 to 127
    bits and r0 >= 2^127 > r1: per size of t1, `per_size` of them.  t1 small makes r0 = (8l - r1 t0) / t1
    large, so the odd combination lat::reduce then forms is wide: max(|c|, d) of 128 to 160 bits."""
    rng = random.Random(seed)
    out = []
    for bits in range(96, 128):
        have = 0
        while have < per_size:
            t1 = rng.randrange(1 << (bits - 1), 1 << bits) & ~1
            t0 = rng.randrange(1, t1) | 1
            if math.gcd(t0, t1) != 1 or math.gcd(t0, L) != 1:
                continue
            r1 = N * pow(t0, -1, t1) % t1
            r0, rem = divmod(N - r1 * t0, t1)
            assert rem == 0
            if not (r0 >= 1 << 127 > r1):
                continue
            k = r0 * pow(t0, -1, N) % N
            for cand in (k, N - k):
                if cand < L and {(r, abs(t)) for r, t in euclid(cand)} == {(r0, t0), (r1, t1)}:
                    out.append(cand)
                    have += 1
                    break
    return out


def class_counts(widths, oks):
    """Records per bit length of max(|c|, d) among those with ok set, and the number with ok clear."""
    per = {}
    for w, ok in zip(widths, oks):
        if ok:
            per[w] = per.get(w, 0) + 1
    return per, sum(1 for ok in oks if not ok)


def check_population(widths, oks) -> None:
    """The constructed set's condition: every width 128..146 at least 16 times, ok clear at least 64 times."""
    per, failed = class_counts(widths, oks)
    thin = {w: per.get(w, 0) for w in range(128, HALF_BITS + 1) if per.get(w, 0) < 16}
    assert not thin, "bit lengths with fewer than 16 records: %s" % thin
    assert failed >= 64, "only %d records with ok clear" % failed


# ---- digit strings ----------------------------------------------------------------------------
def _signed_digits(x: int, bits: int, count: int):
    """count digits of radix 2^bits, every one but the last in [-2^(bits-1), 2^(bits-1)); the last takes
    what is left (the final carry included)."""
    half, out = 1 << (bits - 1), []
    for _ in range(count - 1):
        d = x & ((1 << bits) - 1)
        if d >= half:
            d -= 1 << bits
        out.append(d)
        x = (x - d) >> bits
    return out + [x]


def digits16(x: int, W: int):
    """recode16: digits 0..W-2 in [-8, 7], digit W-1 (top) in [0, 8], for x < 2^(4W-1), W in 33..37."""
    assert 33 <= W <= 37 and 0 <= x < 1 << (4 * W - 1)
    return _signed_digits(x, 4, W)


def digits256(x: int, ndig: int):
    """recode256: ndig digits in [-128, 127]; the top one stays below 128 for x < 2^(8 ndig - 1) - 2^(8 ndig - 9)
    (the kernels hand it x < 2^(8 ndig - 5): a top digit of 8 at most)."""
    assert 17 <= ndig <= 19 and 0 <= x < 1 << (8 * ndig - 1)
    return _signed_digits(x, 8, ndig)


def digits24(x: int, count: int):
    """recode24<count>: digits in [-2^23, 2^23), the top one unreduced (it absorbs the last carry)."""
    assert count in (5, 6) and x >= 0
    return _signed_digits(x, 24, count)


def digits4(x: int, W: int):
    """geu_recode4: digits 0..W-2 in [-2, 1], digit W-1 (top) in [0, 2], for x < 2^(2W-1), W in 66..74."""
    assert 66 <= W <= 74 and 0 <= x < 1 << (2 * W - 1)
    return _signed_digits(x, 2, W)


def base_digit_model(e: int):
    """base_digits: e = lo + 2^141 hi, lo in six radix-2^24 digits, hi in five."""
    assert 0 <= e < L
    return digits24(e & ((1 << B24_SPLIT) - 1), 6), digits24(e >> B24_SPLIT, 5)


def check_digit_string(digits, bits: int, x: int, top_max: int, what: str = "") -> None:
    """One signed digit string, least significant first: every digit but the last in
    [-2^(bits-1), 2^(bits-1)), the last in [0, top_max], and the digits sum back to x."""
    digits = [int(d) for d in digits]
    half = 1 << (bits - 1)
    assert all(-half <= d < half for d in digits[:-1]), "%s: digit out of range: %s" % (what, digits)
    assert 0 <= digits[-1] <= top_max, "%s: top digit %d outside [0, %d]" % (what, digits[-1], top_max)
    assert sum(d << (bits * i) for i, d in enumerate(digits)) == x, "%s: digits do not sum to x = %d" % (what, x)


def check_base_digits(eb: int, el, eh, d: int, s: int, what: str = "") -> None:
    """eb = d s mod l; the halves' digits sum back to it; every digit but the top of a half in
    [-2^23, 2^23), every |digit| <= 2^23 (the last index of a base24 half)."""
    assert eb == d * s % L, "%s: eb != d s mod l" % what
    el, eh = [int(v) for v in el], [int(v) for v in eh]
    assert len(el) == 6 and len(eh) == 5
    lo = sum(v << (24 * i) for i, v in enumerate(el))
    hi = sum(v << (24 * i) for i, v in enumerate(eh))
    assert lo + (hi << B24_SPLIT) == eb, "%s: digits do not sum to eb" % what
    for half in (el, eh):
        assert all(-(1 << 23) <= v < 1 << 23 for v in half[:-1]), "%s: digit out of range: %s" % (what, half)
        assert 0 <= half[-1] <= 1 << 23, "%s: top digit out of the table: %d" % (what, half[-1])
    assert (el, eh) == base_digit_model(eb), "%s: digits differ from the model" % what


def windows16(bits) -> int:
    """wave_windows: the smallest W in 33..37 with every lane's bit length <= 4W - 1; 38 if none."""
    b = max(bits)
    return next((W for W in range(33, 38) if b <= 4 * W - 1), 38)


def windows4(bits) -> int:
    """wave_windows4: the smallest W in 66..74 with every lane's bit length <= 2W - 1 (74 if none)."""
    b = max(bits)
    return next((W for W in range(66, 74) if b <= 2 * W - 1), 74)


def ndig256(W: int) -> int:
    return (((W | 1) - 1) >> 1) + 1


# ---- edge rows --------------------------------------------------------------------------------
def _rep(unit: int, unit_bits: int, total_bits: int) -> int:
    return sum(unit << i for i in range(0, total_bits + unit_bits, unit_bits)) & ((1 << total_bits) - 1)


def recode_edges(limit_bits: int):
    """Values below 2^limit_bits that force maximal carry chains: 0, 1, 2^limit - 1, 2^j and 2^j - 1 for
    j in 127..146, nibble runs of 7s and 8s, byte runs of 0x7f and 0x80, 24-bit groups of 0x7fffff and
    0x800000, radix-4 runs of 1s, 2s and 3s -- each run whole and cut at every length from 120 bits up."""
    cap = 1 << limit_bits
    xs = [0, 1, cap - 1]
    for j in range(127, HALF_BITS + 1):
        xs += [1 << j, (1 << j) - 1]
    for unit, ub in ((7, 4), (8, 4), (0x7F, 8), (0x80, 8), (0x7FFFFF, 24), (0x800000, 24), (1, 2), (2, 2), (3, 2),
                     (0x78, 8), (0x87, 8)):
        for total in range(120, limit_bits + 1):
            xs.append(_rep(unit, ub, total))
        xs.append(_rep(unit, ub, 100) | (1 << (limit_bits - 1)))       # a run below, the top bit set
    return sorted({x for x in xs if 0 <= x < cap})


def base_digit_edges(seed: int):
    """(d, s) rows of base_digits: e = d s mod l is chosen and s = e / d mod l solved for an odd d.
    e: 0, 1, l - 1, 2^141 - 1, 2^141, the runs of recode_edges at 24-bit and other groupings on either
    side of the split; d: 1, 2^146 - 1 and every bit length 128..146; and s = l - 1 with every d."""
    rng = random.Random(seed)
    es = [0, 1, L - 1, (1 << 141) - 1, 1 << 141, (1 << 141) + 1, (1 << 252) - 1, 1 << 252]
    for unit, ub in ((0x7FFFFF, 24), (0x800000, 24), (0xFFFFFF, 24), (0x7F, 8), (0x80, 8), (7, 4), (8, 4)):
        lo = _rep(unit, ub, 141)
        hi = _rep(unit, ub, 111)
        es += [lo, lo | (1 << 140), hi << 141, (hi << 141) | lo, ((hi << 141) | lo) & ((1 << 252) - 1)]
        es += [_rep(unit, ub, 24 * j) for j in range(1, 6)]           # a run that ends at a digit boundary
        es += [_rep(unit, ub, 24 * j) << 141 for j in range(1, 5)]
    es = [e % L for e in es]
    ds = [1, (1 << HALF_BITS) - 1, 3]
    ds += [(1 << (b - 1)) | 1 for b in range(128, HALF_BITS + 1)]
    ds += [rng.randrange(1 << (b - 1), 1 << b) | 1 for b in range(128, HALF_BITS + 1)]
    rows = []
    for i, e in enumerate(es):
        for d in (ds[i % len(ds)], ds[(3 * i + 1) % len(ds)], rng.choice(ds)):
            rows.append((d, e * pow(d, -1, L) % L))
    rows += [(d, L - 1) for d in ds]
    return rows


def random_base_rows(seed: int, n: int = 4000):
    """(d, s): d odd of every bit length 1..146 (128..146 most often), s uniform below l."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        b = 128 + i % 19 if i % 4 else 1 + i % 127
        d = (rng.randrange(1 << (b - 1), 1 << b) if b > 1 else 1) | 1
        rows.append((d, rng.randrange(L)))
    return rows


# ---- ladders ----------------------------------------------------------------------------------
T_VALUES = (0, 0, 1, 2, L - 1, 7)
WIDTH_CLASSES = [127] + list(range(128, HALF_BITS + 1))      # 127 stands for "at most 127 bits"


def t_points():
    """t B for the t of T_VALUES, affine."""
    return {t: ref.pt_mul(t, ref.BASEPOINT) if t else (0, 1) for t in set(T_VALUES)}


def _of_width(rng, cls: int, odd: bool) -> int:
    b = rng.randrange(1, 128) if cls == 127 else cls
    v = rng.randrange(1 << (b - 1), 1 << b)
    return v | 1 if odd else v


def ladder_scalars(seed: int):
    """(|c|, c_neg, d) over the grid of widths {<= 127, 128, .., 146} x the same, both signs of c twice
    over, then edge rows as c and as d: about 2,000 rows, d odd throughout."""
    rng = random.Random(seed)
    rows = []
    for rep in range(2):
        for cw in WIDTH_CLASSES:
            for dw in WIDTH_CLASSES:
                for neg in (0, 1):
                    rows.append((_of_width(rng, cw, False), neg, _of_width(rng, dw, True)))
    edges = recode_edges(HALF_BITS)
    pick = [0, 1, (1 << HALF_BITS) - 1] + rng.sample(edges, 150)
    for i, e in enumerate(pick):
        rows.append((e, (i & 1) if e else 0, _of_width(rng, rng.choice(WIDTH_CLASSES), True)))
        rows.append((_of_width(rng, rng.choice(WIDTH_CLASSES), False), (i >> 1) & 1, e | 1))
    return rows


def ladder_records(seed: int, secrets):
    """Per row of ladder_scalars: a key index into `secrets` (the keys' secret scalars a, A = a B), a
    nonce scalar r (R = r B), t = T_VALUES[i % 6] and the s with d s = c a + d r + t (mod l), so that
    (d s mod l) B - c A - d R = t B.  Returns a list of dicts."""
    rng = random.Random(seed + 1)
    nonces = [rng.randrange(1, L) for _ in range(24)]
    recs = []
    for i, (c_abs, neg, d) in enumerate(ladder_scalars(seed)):
        c = -c_abs if neg else c_abs
        key = rng.randrange(len(secrets))
        r = nonces[i % len(nonces)]
        t = T_VALUES[i % len(T_VALUES)]
        s = (c * secrets[key] + d * r + t) * pow(d, -1, L) % L
        recs.append(dict(c=c_abs, c_neg=neg, d=d, key=key, r=r, t=t, s=s,
                         bits=max(c_abs.bit_length(), d.bit_length())))
    return recs


def limb_value(limbs) -> int:
    offs = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
    return sum(int(v) << o for v, o in zip(limbs, offs)) % P


def check_ladder_record(xyz, ident: int, W: int, want_point, want_W: int, bound, what: str = ""):
    """One ladder result: 30 limbs (X, Y, Z) within `bound` (per limb; negative limbs allowed only when
    the bound array is for the signed field), Z != 0, the point `want_point` projectively, ident set
    exactly when that point is the identity, and the window count.  Returns (X, Y, Z) mod p."""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(3, 10)
    assert (np.abs(xyz) <= np.asarray(bound, dtype=np.int64).reshape(3, 10)).all(), "%s: limb out of bound" % what
    X, Y, Z = (limb_value(v) for v in xyz)
    assert Z != 0, "%s: Z = 0" % what
    x, y = want_point
    assert (X - x * Z) % P == 0 and (Y - y * Z) % P == 0, "%s: wrong point" % what
    assert int(ident) == (1 if (x % P, y % P) == (0, 1) else 0), "%s: ident = %d" % (what, ident)
    assert int(W) == want_W, "%s: W = %d, the model says %d" % (what, W, want_W)
    return X, Y, Z


def same_projective(a, b) -> bool:
    (X1, Y1, Z1), (X2, Y2, Z2) = a, b
    return (X1 * Z2 - X2 * Z1) % P == 0 and (Y1 * Z2 - Y2 * Z1) % P == 0


# ---- host builds ------------------------------------------------------------------------------
def host_lattice():
    """The host build of lattice.h (tests/cpp/lattice_host.cpp), as tests/test_lattice_host.py builds it."""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "tests", "cpp", "build", "liblattice_host.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(root, "narwhal_amd", "csrc"),
                    "-o", so + ".tmp%d" % os.getpid(), os.path.join(root, "tests", "cpp", "lattice_host.cpp")], check=True)
    os.replace(so + ".tmp%d" % os.getpid(), so)
    return ctypes.CDLL(so)


def host_reduce(lib, k: int, fn: str = "lat_reduce"):
    """(|c|, d, c_neg, ok) of the host build."""
    import ctypes
    kw = (ctypes.c_uint32 * 8)(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    c, d = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
    cn, ok = ctypes.c_int(), ctypes.c_int()
    getattr(lib, fn)(kw, c, d, ctypes.byref(cn), ctypes.byref(ok))
    return (sum(c[i] << (32 * i) for i in range(5)), sum(d[i] << (32 * i) for i in range(5)), int(cn.value != 0),
            int(ok.value != 0))
