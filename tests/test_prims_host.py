"""The checks of tests/test_gpu_prims.py, tested without a device.

  * the probe library (tests/hip/prim_probe.hip) cross-compiles from a clean tree with the library's
    flags, exports every entry the ctypes wrapper declares, and is no source of libnwc.so;
  * every checker of tests/prim_probe.py accepts the integer-computed right answer and rejects one
    wrong answer of each kind: a value off by one, a limb one over tight, a non-canonical encoding of
    the right value, a digit out of range, a flipped ok;
  * the call-site classes of the shared group formulas (ge25519.h, ge_sliced.h; the signed-field
    counterpart of tests/test_feu_host.py's MUL_SITES): at the absolute maxima of every (left, right)
    class pair, in Python integers, no prepared operand reaches 2^31, no column 2^63, and the carries
    stay below what the comments of fe_carry_wide / fes_mul say.  A new call site with a new pair of
    classes has to be added to FE_MUL_SITES / FES_MUL_SITES (tests/prim_probe.py), which also puts it
    into the GPU operand rows.
"""
import random
import subprocess

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import prim_probe as pp

P, L = pp.P, pp.L


# ---- probe build ------------------------------------------------------------------------------
def test_probe_builds_and_exports_every_entry(tmp_path):
    from narwhal_amd import build as nb
    out = pp.build_probe(out=str(tmp_path / "libnwc_probe.so"), force=True)
    assert pp.embedded_probe_id(out) == pp.probe_source_id()
    assert pp.probe_up_to_date(out)
    syms = subprocess.run(["nm", "-D", "--defined-only", out], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert set(pp.ENTRIES) | {"probe_record_words", "probe_build_id"} <= exported, sorted(set(pp.ENTRIES) - exported)
    # the probe's table of record sizes is the wrapper's
    src = open(pp.SRC).read()
    for name in pp.ENTRIES:
        assert 'PROBE(%s,' % name in src and '{"%s",' % name in src, name
    # the library's build id does not depend on the probe: no file under tests/ is a source of libnwc.so
    assert all("tests" not in s.split("/") for s in nb.sources())
    assert pp.SRC not in nb.sources()


def test_a_stale_probe_is_told_apart(tmp_path):
    stale = tmp_path / "stale.so"
    stale.write_bytes(b"\x7fELF....NWC_PROBE_ID:0123456789abcdef0123\0....")
    assert pp.embedded_probe_id(str(stale)) == "0123456789abcdef0123"
    assert not pp.probe_up_to_date(str(stale))
    assert not pp.probe_up_to_date(str(tmp_path / "missing.so"))


# ---- checker self-test ------------------------------------------------------------------------
def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def test_field_checkers_accept_right_and_reject_wrong():
    rng = random.Random(1)
    xs = [rng.randrange(P) for _ in range(50)] + [0, 1, P - 1]
    good = np.array([pp.centred_limbs(x) for x in xs], dtype=np.int64)
    pp.check_field(good, xs, pp.TIGHT, "good")
    pp.check_field(good, [x + 3 * P for x in xs], pp.TIGHT, "good mod p")
    off = good.copy(); off[7, 0] += 1                           # a value off by one
    rejects(pp.check_field, off, xs, pp.TIGHT)
    over = good.copy()                                          # the right value, 2^26 moved out of limb 3 into limb 2
    over[5, 2] += 1 << 26
    over[5, 3] -= 1
    assert int(pp.values(over[5:6])[0] - xs[5]) % P == 0 and abs(over[5, 2]) > pp.TIGHT[2]
    pp.check_field(over, xs, None, "value still right")
    rejects(pp.check_field, over, xs, pp.TIGHT)
    edge = good.copy(); edge[0] = pp.TIGHT                      # exactly at the bound passes, one over fails
    pp.check_field(edge, [int(pp.values(edge[:1])[0])] + xs[1:], pp.TIGHT)
    edge[0, 9] += 1
    rejects(pp.check_field, edge, [int(pp.values(edge[:1])[0])] + xs[1:], pp.TIGHT)
    # sliced: idle lanes must be zero
    lanes = np.concatenate([good, np.zeros((len(xs), 6), dtype=np.int64)], axis=1)
    pp.check_sliced(lanes, xs, pp.TIGHT)
    leak = lanes.copy(); leak[3, 12] = 1
    rejects(pp.check_sliced, leak, xs, pp.TIGHT)
    bad = lanes.copy(); bad[3, 4] -= 1
    rejects(pp.check_sliced, bad, xs, pp.TIGHT)
    # unsigned limbs
    u = np.array([pp.limbs_of(x) for x in xs], dtype=np.uint32)
    pp.check_unsigned_field(u, xs, pp.FEU_TIGHT)
    big = u.copy(); big[2, 4] += 1 << 26; big[2, 5] -= 1 if big[2, 5] else 0
    rejects(pp.check_unsigned_field, big, xs, pp.FEU_TIGHT)


def test_encoding_checkers_accept_right_and_reject_wrong():
    xs = [0, 1, 18, 19, P - 1, P, P + 1, 2 * P + 5, 12345678901234567890 ** 3]
    pp.check_canonical(pp.to_words([x % P for x in xs], 8), xs, P)
    rejects(pp.check_canonical, pp.to_words([x % P + (1 if i == 4 else 0) for i, x in enumerate(xs)], 8), xs, P)
    # the right value, not canonical: p + 1 for 1
    rejects(pp.check_canonical, pp.to_words([x % P + (P if i == 1 else 0) for i, x in enumerate(xs)], 8), xs, P)
    ss = [0, L - 1, L, L + 1, (1 << 512) - 1]
    pp.check_canonical(pp.to_words([s % L for s in ss], 8), ss, L)
    rejects(pp.check_canonical, pp.to_words([s % L + (L if i == 2 else 0) for i, s in enumerate(ss)], 8), ss, L)
    pp.check_flags(np.array([1, 0, 1], dtype=np.uint32), [True, False, True])
    rejects(pp.check_flags, np.array([1, 1, 1], dtype=np.uint32), [True, False, True])
    rejects(pp.check_flags, np.array([1, 0, 2], dtype=np.uint32), [True, False, True])


def recode(s, bits, windows):
    """Signed digits of s in Python integers."""
    out, carry = [], 0
    for w in range(windows):
        d = ((s >> (bits * w)) & ((1 << bits) - 1)) + carry
        carry = (d + (1 << (bits - 1))) >> bits
        out.append(d - (carry << bits))
    assert carry == 0
    return out


def test_digit_checker_accepts_right_and_rejects_wrong():
    ss = [s for s in pp.recode_inputs(seed=5, n_uniform=50)][:400]
    for bits, windows in [(4, 64), (8, 32), (16, 16)] + pp.RECODE_SHAPES:
        dig = np.array([recode(s, bits, windows) for s in ss], dtype=np.int64)
        pp.check_digits(dig, bits, ss)
        packed = [sum((d + (1 << (bits - 1))) << (bits * i) for i, d in enumerate(row)) for row in dig.tolist()]
        assert (pp.unpack_digits(pp.to_words(packed, 9), bits, windows) == dig).all()
        off = dig.copy(); off[3, 0] += 1                        # a wrong sum
        rejects(pp.check_digits, off, bits, ss)
        row = next(i for i in range(len(ss)) if dig[i, 0] < 0)
        wide = dig.copy()                                       # the right sum, one digit out of range
        wide[row, 0] += 1 << bits
        wide[row, 1] -= 1
        rejects(pp.check_digits, wide, bits, ss)
        top = dig.copy(); top[5, 1] = 1 << (bits - 1)           # 2^(bits-1) itself is out of range
        rejects(pp.check_digits, top, bits, ss)


def decode_record(point, ok, y, small, z=1):
    rec = np.zeros(50, dtype=np.int64)
    if point is not None:
        rec[:40] = pp.ext_limbs(point, z)
    rec[40] = ok
    rec[41:49] = pp.to_words([y], 8)[0]
    rec[49] = small
    return rec


def test_decode_and_point_checkers_accept_right_and_reject_wrong():
    rng = random.Random(3)
    enc = pp.decode_inputs(seed=3, n_points=12, n_random=24)
    reference = pp.decode_reference(enc)
    assert any(r[0] is None for r in reference) and any(r[2] for r in reference)
    good = np.array([decode_record(pt, pt is not None, y, so, rng.randrange(1, P)) for pt, y, so in reference])
    as_words = lambda a: a.astype(np.int32).view(np.uint32)     # noqa: E731
    pp.check_decode(as_words(good), reference, pp.DECODE_TIGHT)
    on = next(i for i, r in enumerate(reference) if r[0] is not None)
    offc = next(i for i, r in enumerate(reference) if r[0] is None)
    for row, col, delta in ((on, 40, -1), (offc, 40, 1),        # a flipped ok, both ways
                            (on, 0, 1),                         # X off by one
                            (on, 30, 1),                        # T off by one: T Z != X Y
                            (on, 49, 1 - 2 * int(good[on, 49])),    # the small-order flag
                            (on, 41, 1)):                       # canonical y off by one
        bad = good.copy(); bad[row, col] += delta
        rejects(pp.check_decode, as_words(bad), reference, pp.DECODE_TIGHT)
    ybig = next(i for i, r in enumerate(reference) if r[1] < 19)   # y + p: the right value, not canonical
    bad = good.copy(); bad[ybig, 41:49] = pp.to_words([reference[ybig][1] + P], 8)[0]
    rejects(pp.check_decode, as_words(bad), reference, pp.DECODE_TIGHT)
    bad = good.copy(); bad[on, 2] += 1 << 26; bad[on, 3] -= 1   # the right point, a limb past tight
    rejects(pp.check_decode, as_words(bad), reference, pp.DECODE_TIGHT)
    # check_points alone: a wrong point that is still on the curve
    pts = pp.group_points()[8:12]
    recs = np.array([pp.ext_limbs(p, rng.randrange(1, P)) for p in pts], dtype=np.int64)
    pp.check_points(recs, pts, (pp.TIGHT,) * 4)
    rejects(pp.check_points, recs, [ref.pt_neg(p) for p in pts], (pp.TIGHT,) * 4)
    zero_z = recs.copy(); zero_z[1, 20:30] = 0
    rejects(pp.check_points, zero_z, pts, (pp.TIGHT,) * 4)


def test_operand_rows_hold_what_the_tests_rely_on():
    rows, tags = pp.signed_pair_rows(pp.CONTRACT_PAIRS, seed=1, n_uniform=200, n_signs=2000, n_mixed=20, n_random=50)
    for left, right in pp.CONTRACT_PAIRS:
        blk = rows[tags == "%s:%s" % (left, right)]
        m = np.concatenate([pp.SIGNED_CLASSES[left], pp.SIGNED_CLASSES[right]])
        assert (np.abs(blk) <= m).all()
        at_max = blk[(np.abs(blk) == m).all(axis=1)]
        assert len(np.unique(np.sign(at_max), axis=0)) >= 2000  # distinct sign patterns at the maxima
        assert (at_max > 0).all(axis=1).any() and (at_max < 0).all(axis=1).any()
    a, va, vb = pp.canon_rows(seed=2, n=3000)
    assert ((pp.values(a[:, :10]) - va) % P == 0).all() and ((pp.values(a[:, 10:]) - vb) % P == 0).all()
    assert (np.abs(a[:, :10]) <= 7 * pp.TIGHT).all() and (np.abs(a[:, 10:]) <= pp.TIGHT).all()
    assert {int(v) % P for v in va} >= {0, 1, P - 1, 18, 19, 20, P - 19, P - 20}
    assert all(x < 1 << 253 for x in pp.recode_inputs(seed=5, n_uniform=10))
    xs = pp.reduce_inputs(seed=4, n_uniform=10)
    assert all(0 <= x < 1 << 512 for x in xs) and {0, L, L - 1, L + 1, (1 << 512) - 1} <= set(xs)
    for x in (0, 1, P - 1, P + 5, 2 ** 254 + 12345):
        assert int(pp.values(np.array([pp.centred_limbs(x)]))[0]) % P == x % P
        assert (np.abs(pp.centred_limbs(x)) <= pp.TIGHT).all()


# ---- call-site classes ------------------------------------------------------------------------
BIAS = [1 << (w - 1) for w in pp.WID]


def columns(f, g, scale=1):
    """Largest |column| + bias of the schoolbook product at per-limb maxima f, g: column k collects
    f_i g_j, i + j = k mod 10, x 19 where it wraps, x 2 where i and j are both odd."""
    cols = []
    for k in range(10):
        h = 0
        for i in range(10):
            j = (k - i) % 10
            h += int(f[i]) * int(g[j]) * (19 if i > k else 1) * (2 if i & 1 and j & 1 else 1)
        cols.append(scale * h + BIAS[k])
    return cols


def carry_wide(cols):
    """fe_carry_wide's two interleaved chains on column magnitudes: the carries that are added into
    32-bit words (limb 5's and limb 1's) and the largest limb magnitudes that come out."""
    h = list(cols)
    c = lambda k: (h[k] >> pp.WID[k]) + 1                       # noqa: E731  |floor carry| <= this
    h[1] += c(0); h[5] += c(4); h[2] += c(1); h[6] += c(5); h[3] += c(2); h[7] += c(6)
    h4 = (1 << 26) + c(3)
    h[8] += c(7)
    into5 = (h4 >> 26) + 1
    h[9] += c(8)
    h0 = (1 << 26) + 19 * c(9)
    into1 = (h0 >> 26) + 1
    limbs = list(BIAS)
    limbs[5] += into5
    limbs[1] += into1
    return into5, into1, limbs


def sliced_carries(cols):
    """fes_mul's two parallel rounds: round 1's carries, round 2's, and the output limb magnitudes."""
    c1 = [(h >> w) + 1 for h, w in zip(cols, pp.WID)]
    cin = [19 * c1[9]] + c1[:9]
    c2 = [(((1 << w) + x) >> w) + 1 for x, w in zip(cin, pp.WID)]
    cin2 = [19 * c2[9]] + c2[:9]
    return c1, c2, [b + x for b, x in zip(BIAS, cin2)]


@pytest.mark.parametrize("left,right", pp.FE_MUL_SITES + pp.CONTRACT_PAIRS)
def test_fe_mul_sites_hold_at_their_maxima(left, right):
    f, g = pp.SIGNED_CLASSES[left], pp.SIGNED_CLASSES[right]
    assert all(19 * int(x) < 1 << 31 for x in g), "19 g"
    assert all(2 * int(f[i]) < 1 << 31 for i in (1, 3, 5, 7, 9)), "2 f_odd"
    cols = columns(f, g)
    assert max(cols) < 1 << 63
    into5, into1, limbs = carry_wide(cols)
    assert into5 < 1 << 12 and into1 < 1 << 17               # fe_carry_wide: "c < 2^12 here", "c < 2^17 here"
    assert all(l <= t for l, t in zip(limbs, pp.TIGHT))


@pytest.mark.parametrize("cls", pp.FE_SQ_SITES + ["L"])
def test_fe_sq_sites_hold_at_their_maxima(cls):
    f = pp.SIGNED_CLASSES[cls]
    assert all(38 * int(f[i]) < 1 << 31 for i in (1, 3, 5, 7, 9)), "38 f_odd"
    assert all(19 * int(f[i]) < 1 << 31 and 2 * int(f[i]) < 1 << 31 for i in range(10))
    cols = columns(f, f)
    assert max(cols) < 1 << 63
    into5, into1, limbs = carry_wide(cols)
    assert into5 < 1 << 12 and into1 < 1 << 17
    assert all(l <= t for l, t in zip(limbs, pp.TIGHT))


@pytest.mark.parametrize("cls", pp.FE_SQ2_SITES + ["L"])
def test_fe_sq2_sites_hold_at_their_maxima(cls):
    f = pp.SIGNED_CLASSES[cls]
    assert all(38 * int(f[i]) < 1 << 31 for i in (1, 3, 5, 7, 9)), "38 f_odd"
    assert all(4 * int(x) < 1 << 31 for x in f), "4 f"
    cols = columns(f, f, scale=2)
    assert max(cols) < 1 << 63
    into5, into1, limbs = carry_wide(cols)
    assert into5 < 1 << 12 and into1 < 1 << 17
    assert all(l <= t for l, t in zip(limbs, pp.TIGHT))


@pytest.mark.parametrize("left,right", pp.FES_MUL_SITES + pp.CONTRACT_PAIRS)
def test_fes_mul_sites_hold_at_their_maxima(left, right):
    f, g = pp.SIGNED_CLASSES[left], pp.SIGNED_CLASSES[right]
    assert all(19 * int(x) < 1 << 31 for x in g), "19 g"        # the 19 and the 2 both sit on g
    assert all(38 * int(g[i]) < 1 << 31 for i in (1, 3, 5, 7, 9)), "38 g_odd"
    cols = columns(f, g)
    assert max(cols) < 1 << 62                                  # fe_sliced.h: "column sums stay below 2^62"
    c1, c2, limbs = sliced_carries(cols)
    assert max(c1) <= 1 << 37                                   # round 1: "up to 2^37"
    assert max(c2[1:]) <= 1 << 12 and c2[0] < 1 << 16           # round 2: 2^12 (x 19 into limb 0); limb 0's own, into limb 1
    assert all(l <= t for l, t in zip(limbs, pp.TIGHT))


def test_fe_mul_small_and_fes_mul_small_at_their_maxima():
    f = pp.LOOSE
    cols = [int(x) * 31 + b for x, b in zip(f, BIAS)]           # fe_mul_small: |c| < 2^5, through fe_carry_wide
    into5, into1, limbs = carry_wide(cols)
    assert all(l <= t for l, t in zip(limbs, pp.TIGHT))
    for cls, c in (("L", (1 << 17) - 1), ("2T", 121666)):       # the contract; gs_xonly_dbl_n's 121666 e
        f = pp.SIGNED_CLASSES[cls]
        cy = [((int(x) * c + b) >> w) + 1 for x, b, w in zip(f, BIAS, pp.WID)]
        assert max(cy) < 1 << 18                                # "carries up to 2^18, x 19 into limb 0"
        assert abs(19 * cy[9]) < 1 << 31
        out = [b + x for b, x in zip(BIAS, [19 * cy[9]] + cy[:9])]
        assert all(o <= m for o, m in zip(out, pp.FES_SMALL_OUT))


def test_the_acc_conversions_remark():
    """ge_p1p1_to_p2_acc / _to_p3_acc put Y on the right: 19 Y fits for a sum of two tight elements
    (2^30.3) and not for twice that, which is why the Niels path keeps the plain conversions."""
    two, four = pp.SIGNED_CLASSES["2T"], 4 * pp.TIGHT
    assert all(19 * int(x) < 1 << 31 for x in two)
    assert max(19 * int(x) for x in two) < 2 ** 30.31
    assert any(19 * int(x) >= 1 << 31 for x in four)
    assert ("3T", "2T") in pp.FE_MUL_SITES


def test_site_pairs_are_in_the_gpu_operand_rows():
    rows, tags = pp.signed_pair_rows(pp.FE_MUL_SITES + pp.FES_MUL_SITES, seed=1, n_uniform=10, n_signs=10, n_mixed=5,
                                     n_random=5)
    assert {"%s:%s" % s for s in pp.FE_MUL_SITES + pp.FES_MUL_SITES} <= set(tags.tolist())
    assert all(c in ("T", "2T", "3T", "RAW") for c in pp.FE_SQ_SITES + pp.FE_SQ2_SITES)   # left classes of those rows
