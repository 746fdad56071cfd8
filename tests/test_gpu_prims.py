"""Unit tests of the device-only primitives, on the device: the signed field (fe25519.h, fe_asm.h), the
limb-sliced field and group (fe_sliced.h, ge_sliced.h), the asm half of the unsigned field (feu_asm.h),
the scalars (sc25519.h) and point decoding (ge25519.h, ge_u25519.h).

Every other GPU test judges this arithmetic by one bit per signature.  Here each primitive runs alone
through the probe library (tests/hip/prim_probe.hip, built by __graft_entry__.build() with the
library's own flags) and is compared exactly with Python integers and oracle/ed25519_ref.py: field
results mod p, scalars and encodings bit for bit, and output limbs against the bound the headers
promise.  Nothing here takes a tolerance.  The operand rows sit where such code goes wrong: every
limb at +- its class maximum in thousands of sign patterns, values within 19 of a multiple of p in
non-canonical limbs, q l - 1 / q l / q l + 1 for Barrett, runs of maximal digits for the recodings.
The rows, the checkers and the call-site classes live in tests/prim_probe.py; tests/test_prims_host.py
tests the checkers and the classes without a device.

Every record set is launched whole (more than one 256-lane block, a ragged last wave) and again as
its first 1, 63, 64, 65 and 257 records (sliced probes: 1..5 and 7 rows, so rows of the last wave
idle); a short launch must reproduce the whole launch's words.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import prim_probe as pp
from tests import test_feu_host as feu_host
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

P, L = pp.P, pp.L


@pytest.fixture(scope="module", autouse=True)
def probe():
    return pp.load()        # a missing or stale probe library is an error, not a skip


def report(family, records, edge):
    print("%s: %d records, %d of them edge rows" % (family, records, edge))


def i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int32))


def merge_sites(*lists):
    out = []
    for pair in [p for lst in lists for p in lst]:
        if pair not in out:
            out.append(pair)
    return out


# ---- signed field -----------------------------------------------------------------------------
def test_signed_field_products():
    """fe_mul, fe_sq, fe_sq2, fe_mul_small: value mod p and tight output limbs on tight / loose operands
    and on every call-site class pair of ge25519.h."""
    rows, tags = pp.signed_pair_rows(merge_sites(pp.CONTRACT_PAIRS, pp.FE_MUL_SITES), seed=1)
    c = pp.small_constants(len(rows), 32, seed=11)
    assert {31, -31, 0, 1, -1} <= set(c.tolist())
    rec = pp.ragged(i32(np.concatenate([rows, c[:, None]], axis=1)), "probe_fe_ops")
    out = pp.run_whole_and_ragged("probe_fe_ops", rec, pp.LANE_COUNTS)
    lim = pp.signed(rec)
    f, g, cc = pp.values(lim[:, :10]), pp.values(lim[:, 10:20]), lim[:, 20].astype(object)
    res = pp.signed(out)
    pp.check_field(res[:, 0:10], f * g, pp.TIGHT, "fe_mul")
    pp.check_field(res[:, 10:20], f * f, pp.TIGHT, "fe_sq")
    pp.check_field(res[:, 20:30], 2 * f * f, pp.TIGHT, "fe_sq2")
    pp.check_field(res[:, 30:40], f * cc, pp.TIGHT, "fe_mul_small")
    report("signed field products", len(rec), int((tags != "RAW:RAW").sum()) + 361)


def test_signed_field_words_and_tighten():
    """fe_from_words, fe_tighten and fe_to_words on 256-bit strings: bit 255 ignored, y >= p reduced."""
    w = pp.ragged(pp.word_rows(seed=3), "probe_fe_words")
    out = pp.run_whole_and_ragged("probe_fe_words", w, pp.LANE_COUNTS)
    y = np.array([int(v) & ((1 << 255) - 1) for v in pp.words_value(w)], dtype=object)
    want = np.array([pp.limbs_of(int(v)) for v in y], dtype=np.int64)
    assert (pp.signed(out[:, 0:10]) == want).all(), "fe_from_words"
    pp.check_field(pp.signed(out[:, 10:20]), y, pp.TIGHT, "fe_tighten")
    pp.check_canonical(out[:, 20:28], y, P, "fe_to_words")
    report("signed field words", len(w), len(w) - 8000)


def test_signed_field_canonical_encoding():
    """fe_to_words, fe_is_zero, fe_is_negative, fe_equal on non-canonical limbs of values within 20 of
    a multiple of p, up to the 8 x tight the header says they accept."""
    rows, va, vb = pp.canon_rows(seed=2)
    assert len(rows) >= 50000
    assert (np.abs(rows[:, :10]) > 4 * pp.TIGHT).any(axis=1).sum() > 10000
    rec = pp.ragged(i32(rows), "probe_fe_canon")
    if len(rec) > len(rows):
        va, vb = np.append(va, va[0]), np.append(vb, vb[0])
    out = pp.run_whole_and_ragged("probe_fe_canon", rec, pp.LANE_COUNTS)
    pp.check_canonical(out[:, 0:8], va, P, "fe_to_words")
    zero = [int(v) % P == 0 for v in va]
    assert sum(zero) > 3000
    pp.check_flags(out[:, 8], zero, "fe_is_zero")
    pp.check_flags(out[:, 9], [(int(v) % P) & 1 for v in va], "fe_is_negative")
    equal = [(int(a) - int(b)) % P == 0 for a, b in zip(va, vb)]
    assert 10000 < sum(equal) < len(equal) - 10000
    pp.check_flags(out[:, 10], equal, "fe_equal")
    report("canonical encoding", len(rec), len(rec))


def power_rows(seed):
    """Operands of the exponentiation chains: 0, +-1, small values, p - 1 as decoded, uniform values as
    tight and as decoded limbs, and loose / 2 x tight / 3 x tight limbs at and inside their maxima."""
    nrng = np.random.default_rng(seed)
    import random
    rng = random.Random(seed)
    rows = [[0] * 10, pp.centred_limbs(1), pp.centred_limbs(-1), pp.centred_limbs(2), pp.limbs_of(P - 1),
            pp.limbs_of(P), pp.limbs_of((1 << 255) - 1), pp.centred_limbs(ref.SQRT_M1)]
    rows += [pp.centred_limbs(rng.randrange(P)) for _ in range(1800)]
    rows += [pp.limbs_of(rng.randrange(P)) for _ in range(600)]
    parts = [np.array(rows, dtype=np.int64)]
    for cls in ("L", "2T", "3T"):
        m = pp.SIGNED_CLASSES[cls]
        parts.append((nrng.integers(0, 2, size=(300, 10)) * 2 - 1) * m)
        parts.append(nrng.integers(-m, m + 1, size=(300, 10)))
    return np.concatenate(parts)


def test_signed_field_powers():
    """fe_pow22523 against pow(z, 2^252 - 3, p); fe_invert: result x input = 1, and 0 for the zero input."""
    rows = pp.ragged(i32(power_rows(5)), "probe_fe_pow")
    out = pp.run_whole_and_ragged("probe_fe_pow", rows, pp.LANE_COUNTS)
    z = pp.values(pp.signed(rows))
    res = pp.signed(out)
    pp.check_field(res[:, 0:10], [pow(int(v) % P, 2**252 - 3, P) for v in z], pp.TIGHT, "fe_pow22523")
    inv = pp.values(res[:, 10:20])
    assert all((int(a) * int(b) - (1 if int(b) % P else 0)) % P == 0 for a, b in zip(inv, z)), "fe_invert"
    pp.check_field(res[:, 10:20], [pow(int(v) % P, P - 2, P) for v in z], pp.TIGHT, "fe_invert")
    assert int(inv[0]) % P == 0
    report("signed field powers", len(rows), 8 + 1800)


# ---- sliced field -----------------------------------------------------------------------------
def test_sliced_field_products():
    """fes_mul, fes_sq, fes_mul_small and the fes_from_fe / fe_from_fes round trip, four different
    elements per wave; every fourth wave row all zero next to one at the loose maxima."""
    rows, tags = pp.signed_pair_rows(merge_sites(pp.CONTRACT_PAIRS, pp.FES_MUL_SITES), seed=7)
    c = pp.small_constants(len(rows), 1 << 17, seed=17)
    assert {(1 << 17) - 1, -((1 << 17) - 1), 0, 1, -1} <= set(c.tolist())
    body = np.concatenate([rows, c[:, None]], axis=1)
    # leak rows: waves of (a row, all zero, the maxima, a row); a zero row must come out all zero
    k = 1500
    peak = np.concatenate([pp.LOOSE, -pp.LOOSE, [(1 << 17) - 1]])
    alt = np.concatenate([pp.LOOSE * np.array([1, -1] * 5), pp.LOOSE, [-((1 << 17) - 1)]])
    leak = np.zeros((4 * k, 21), dtype=np.int64)
    leak[0::4] = body[-2 * k::2]
    leak[2::4] = np.where((np.arange(k) % 2 == 0)[:, None], peak, alt)
    leak[3::4] = body[-2 * k + 1::2]
    rec = pp.ragged(i32(np.concatenate([leak, body])), "probe_fes_ops")
    out = pp.run_whole_and_ragged("probe_fes_ops", rec, pp.ROW_COUNTS)
    assert (out[1:4 * k:4] == 0).all(), "a zero row picked something up from its wave"
    lim = pp.signed(rec)
    f, g, cc = pp.values(lim[:, :10]), pp.values(lim[:, 10:20]), lim[:, 20].astype(object)
    res = pp.signed(out)
    pp.check_sliced(res[:, 0:16], f * g, pp.TIGHT, "fes_mul")
    pp.check_sliced(res[:, 16:32], f * f, pp.TIGHT, "fes_sq")
    pp.check_sliced(res[:, 32:48], f * cc, pp.FES_SMALL_OUT, "fes_mul_small")
    assert (res[:, 48:58] == lim[:, :10]).all() and (res[:, 58:64] == 0).all(), "fes_from_fe"
    assert (res[:, 64:80] == lim[:, 10 + np.arange(16) % 10]).all(), "fe_from_fes"
    report("sliced field products", len(rec), 4 * k + int((tags != "RAW:RAW").sum()) + 361)


def test_sliced_field_power():
    rows = pp.ragged(i32(power_rows(9)), "probe_fes_pow")
    out = pp.run_whole_and_ragged("probe_fes_pow", rows, pp.ROW_COUNTS)
    z = pp.values(pp.signed(rows))
    pp.check_sliced(pp.signed(out), [pow(int(v) % P, 2**252 - 3, P) for v in z], pp.TIGHT, "fes_pow22523")
    report("sliced field power", len(rows), 8 + 1800)


def test_sliced_group():
    """gs_dbl and gs_add_cached (through gs_to_p3) and gs_has_torsion on the small-order points, multiples
    of B and mixed-order points under random Z, one point pair per wave; all four rows of the wave
    hold the result."""
    import random
    rng = random.Random(31)
    pts = pp.group_points()
    pairs = [(p, q) for p in pts for q in pts]
    rec = i32([pp.ext_limbs(p, rng.randrange(1, P)) + pp.ext_limbs(q, rng.randrange(1, P)) for p, q in pairs])
    rec = pp.ragged(rec, "probe_gs")
    pairs = pairs + pairs[:len(rec) - len(pairs)]
    out = pp.run_whole_and_ragged("probe_gs", rec, (1, 2, 3, 5)).reshape(len(rec), 4, 81)
    assert (out == out[:, :1, :]).all(), "the four rows of a wave disagree"
    res = pp.signed(out[:, 0, :])
    bounds = (pp.TIGHT,) * 4
    pp.check_points(res[:, 0:40], [ref.pt_add(p, p) for p, _ in pairs], bounds, "gs_dbl")
    pp.check_points(res[:, 40:80], [ref.pt_add(p, q) for p, q in pairs], bounds, "gs_add_cached")
    tor = {p: ref.has_torsion(p) for p in pts}
    assert sum(tor.values()) == 9                       # 7 small-order points but the identity, 2 mixed
    pp.check_flags(res[:, 80], [tor[p] for p, _ in pairs], "gs_has_torsion")
    report("sliced group", len(rec), len(rec))


# ---- per-lane group layer ---------------------------------------------------------------------
def test_group_ops():
    """ge25519.h one operation at a time, one point pair per lane: ge_p2_dbl through the four p1p1
    conversions, ge_add_cached and ge_add_niels with and without the conditional negation, ge_p3_neg.
    The pairs are all of group_points() x group_points() (the identity, the small-order points,
    multiples of B, mixed-order points; P = Q on the diagonal) and (P, -P) for every P, under random
    Z; P and Q come tight -- in 64 further records with one coordinate each at +- the tight maximum in
    every limb -- and the Niels operand in the three classes a table entry comes in (as built, carried,
    at the edge of 2 x tight).  Every output coordinate is a product: tight."""
    import random
    rng = random.Random(41)
    pts = pp.group_points()
    pairs = [(p, q) for p in pts for q in pts] + [(p, ref.pt_neg(p)) for p in pts]
    assert sum(p == q for p, q in pairs) >= len(pts) and sum(ref.pt_add(p, q) == (0, 1) for p, q in pairs) >= len(pts)
    rows = [pp.ext_limbs(p, rng.randrange(1, P)) + pp.ext_limbs(q, rng.randrange(1, P)) + pp.niels_limbs(q, i % 3, rng)
            for i, (p, q) in enumerate(pairs)]
    # the tight class at its edge: one coordinate of P and one of Q at +- the tight maximum in every limb
    # (the scale Z is chosen for it), every coordinate in turn, on every kind of point
    edge = [(pts[(5 * i) % len(pts)], pts[(7 * i + 3) % len(pts)]) for i in range(64)]
    rows += [pp.ext_limbs_at_maxima(p, i % 4, rng) + pp.ext_limbs_at_maxima(q, (i // 4) % 4, rng) + pp.niels_limbs(q, i % 3, rng)
             for i, (p, q) in enumerate(edge)]
    pairs += edge
    rec = i32(rows)
    lim = pp.signed(rec)
    at_max = (np.abs(lim[len(rows) - 64:, :80].reshape(-1, 10)) == pp.TIGHT).all(axis=1).reshape(64, 8)
    assert (at_max.sum(axis=1) >= 2).all() and at_max[:, :4].any(axis=0).all() and at_max[:, 4:].any(axis=0).all()
    assert (np.abs(lim[:, :80].reshape(-1, 10)) <= pp.TIGHT).all()
    assert (np.abs(lim[:, 80:100].reshape(-1, 10)) <= 2 * pp.TIGHT).all() and (np.abs(lim[:, 100:110]) <= pp.TIGHT).all()
    assert (np.abs(lim[2::3, 80:100].reshape(-1, 10)).max(axis=0) > 1.5 * pp.TIGHT).all()   # form 2 goes well past tight in every limb
    rec = pp.ragged(rec, "probe_ge_ops")
    pairs = pairs + pairs[:len(rec) - len(pairs)]
    out = pp.signed(pp.run_whole_and_ragged("probe_ge_ops", rec, pp.LANE_COUNTS))
    t4, t3 = (pp.TIGHT,) * 4, (pp.TIGHT,) * 3
    dbl = [ref.pt_add(p, p) for p, _ in pairs]
    add = [ref.pt_add(p, q) for p, q in pairs]
    sub = [ref.pt_add(p, ref.pt_neg(q)) for p, q in pairs]
    pp.check_points(out[:, 0:40], dbl, t4, "ge_p1p1_to_p3(ge_p2_dbl)")
    pp.check_p2(out[:, 40:70], dbl, t3, "ge_p1p1_to_p2(ge_p2_dbl)")
    pp.check_points(out[:, 70:110], dbl, t4, "ge_p1p1_to_p3_acc(ge_p2_dbl)")
    pp.check_p2(out[:, 110:140], dbl, t3, "ge_p1p1_to_p2_acc(ge_p2_dbl)")
    pp.check_points(out[:, 140:180], add, t4, "ge_add_cached")
    pp.check_points(out[:, 180:220], sub, t4, "ge_add_cached of ge_cached_cneg")
    pp.check_points(out[:, 220:260], add, t4, "ge_add_niels")
    pp.check_points(out[:, 260:300], sub, t4, "ge_add_niels of ge_niels_cneg")
    pp.check_points(out[:, 300:340], [ref.pt_neg(p) for p, _ in pairs], t4, "ge_p3_neg")
    report("per-lane group layer", len(rec), len(rec))


# ---- unsigned field, device build -------------------------------------------------------------
@pytest.fixture(scope="module")
def feu_plain_exe():
    """tests/cpp/feu_host.cpp without the sanitizers: the same algorithm in plain u64 arithmetic."""
    out = os.path.join(feu_host.BUILD, "feu_host_plain")
    os.makedirs(feu_host.BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + feu_host.CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "feu_host.cpp")], check=True)
    return out


def test_unsigned_field_on_the_device(feu_plain_exe, tmp_path):
    """feu_asm.h's device half on tests/test_feu_host.py's operand rows: limb for limb the host build's
    output, and the host test's own value and tightness checks."""
    ops, tags = feu_host.field_operands()
    ops = pp.ragged(ops, "probe_feu_field")
    tags = list(tags) + list(tags[:len(ops) - len(tags)])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    ops.tofile(fin)
    feu_host.run(feu_plain_exe, ["field", fin, fout])
    host = np.fromfile(fout, dtype=np.uint32).reshape(len(ops), 110)
    dev = pp.run_whole_and_ragged("probe_feu_field", ops, pp.LANE_COUNTS)
    diff = np.nonzero((dev != host).any(axis=1))[0]
    assert diff.size == 0, ("device and host builds differ", diff[:4], [tags[i] for i in diff[:4]])
    feu_host.check_field_output(ops, tags, dev.reshape(len(ops), 11, 10))
    report("unsigned field on the device", len(ops), len(ops) - 40000)


# ---- scalars ----------------------------------------------------------------------------------
def test_scalar_reduce512():
    xs = pp.reduce_inputs(seed=4)
    rec = pp.ragged(pp.to_words(xs, 16), "probe_sc_reduce")
    out = pp.run_whole_and_ragged("probe_sc_reduce", rec, pp.LANE_COUNTS)
    pp.check_canonical(out, pp.words_value(rec), L, "sc_reduce512")
    report("sc_reduce512", len(rec), len(rec) - 20000)


def test_scalar_lt_l():
    import random
    rng = random.Random(6)
    xs = pp.lt_l_inputs()
    edge = len(xs)
    xs += [rng.getrandbits(256) for _ in range(300)] + [L + rng.randrange(-(1 << 130), 1 << 130) for _ in range(300)]
    rec = pp.ragged(pp.to_words(xs, 8), "probe_sc_lt_l")
    out = pp.run_whole_and_ragged("probe_sc_lt_l", rec, pp.LANE_COUNTS)
    pp.check_flags(out, [int(v) < L for v in pp.words_value(rec)], "sc_lt_l")
    report("sc_lt_l", len(rec), edge)


def test_scalar_recodings():
    """The four signed recodings on s < 2^253: digits in range, sum d_i 2^(BITS i) = s, digit_at = the digits."""
    xs = pp.recode_inputs(seed=5)
    rec = pp.ragged(pp.to_words(xs, 8), "probe_sc_recode")
    out = pp.run_whole_and_ragged("probe_sc_recode", rec, pp.LANE_COUNTS)
    s = pp.words_value(rec)
    pp.check_digits(pp.unpack_digits(out[:, 0:8], 4, 64), 4, s, "sc_recode_radix16")
    pp.check_digits(pp.unpack_digits(out[:, 8:16], 8, 32), 8, s, "sc_recode_radix256")
    pp.check_digits(pp.unpack_digits(out[:, 16:24], 16, 16), 16, s, "sc_recode_radix65536")
    at = 24
    for bits, windows in pp.RECODE_SHAPES:
        what = "sc_recode_radix<%d, %d>" % (bits, windows)
        packed, dig = out[:, at:at + 9], pp.signed(out[:, at + 9:at + 9 + windows])
        assert (pp.words_value(packed) >> (bits * windows) == 0).all(), what + ": bits past the last digit"
        pp.check_digits(dig, bits, s, what + " through digit_at")
        assert (pp.unpack_digits(packed, bits, windows) == dig).all(), what + ": digit_at differs from the packed digits"
        at += 9 + windows
    assert at == out.shape[1]
    report("recodings", len(rec), len(rec) - 6000)


# ---- decoding ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_set():
    enc = pp.ragged(pp.decode_inputs(seed=12), "probe_decompress1")
    return enc, pp.decode_reference(enc)


def test_decompress1(decode_set):
    enc, reference = decode_set
    assert 1500 < sum(r[0] is None for r in reference) < 2600
    out = pp.run_whole_and_ragged("probe_decompress1", enc, pp.LANE_COUNTS)
    pp.check_decode(out, reference, pp.DECODE_TIGHT, what="ge_decompress1")
    report("decoding", len(enc), len(enc) - 8000)


def test_decompress2_agrees_with_decompress1(decode_set):
    """ge_decompressN<2> on two different encodings per lane: each slot is ge_decompress1's answer."""
    enc, reference = decode_set
    other = np.roll(np.arange(len(enc)), 37)
    pairs = np.concatenate([enc, enc[other]], axis=1)
    out = pp.run_whole_and_ragged("probe_decompress2", pairs, pp.LANE_COUNTS)
    pp.check_decode(out[:, :50], reference, pp.DECODE_TIGHT, what="ge_decompressN<2> slot 0")
    pp.check_decode(out[:, 50:], [reference[i] for i in other], pp.DECODE_TIGHT, what="ge_decompressN<2> slot 1")
    one = pp.run("probe_decompress1", enc)
    assert (out[:, :50] == one).all() and (out[:, 50:] == one[other]).all()


def test_geu_decompress(decode_set):
    enc, reference = decode_set
    out = pp.run_whole_and_ragged("probe_geu_decompress", enc, pp.LANE_COUNTS)
    pp.check_decode(out, reference, pp.DECODE_FEU, nonneg=True, what="geu_decompress")
