"""The table audit's host side (tests/table_audit.py), tested without a device: the restated audit
passes a reference comb, flags every mutant at exactly the mutated entry and its successor with the
right bit, and the defects it cannot see -- a window of multiples of the wrong point -- are caught by
the exact check of the window's entries 0 and 1.  tests/test_gpu_tables.py runs the same mutants
through the probe's audit kernel and must get the same flags.
"""
import random

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import prim_probe as pp
from tests import table_audit as ta

P = pp.P
BITS, WINDOWS = 4, 3
ENTRIES = (1 << (BITS - 1)) + 1


@pytest.fixture(scope="module")
def comb():
    point = ref.pt_mul(0x1234567, ref.BASEPOINT)
    return point, ta.reference_comb(point, BITS, WINDOWS)


def window_points(point, w):
    return ta.multiples(ta.window_base(point, BITS, w), 0, ENTRIES)


def test_the_reference_comb_passes_both_checks(comb):
    point, words = comb
    assert words.shape == (WINDOWS * ENTRIES, 32)
    assert not ta.flagged(ta.audit_flags(words, WINDOWS, ENTRIES))
    for w in range(WINDOWS):
        ta.check_entries(words[w * ENTRIES:(w + 1) * ENTRIES], window_points(point, w), "window %d" % w)
    # entry j of window w is j 2^(4 w) P, by pt_mul alone
    for w, j in ((0, 1), (1, 1), (2, 8), (1, 5)):
        assert ta.niels_values(ref.pt_mul(j << (BITS * w), point)) == tuple(
            int(v) % P for v in pp.values(ta.entry_parts(words[w * ENTRIES + j:][:1])[0][0]))
    # the unpadded layout of the 129-entry tables: the first 30 words alone
    short = words.copy()
    short[:, 30:] = 0
    assert not ta.flagged(ta.audit_flags(short, WINDOWS, ENTRIES))


def test_the_identity_and_small_order_windows_pass(comb):
    """A comb of a small-order key (its multiples cycle through E[8], the identity included) is as
    valid a table as any: the addition law is complete."""
    for q in ref.small_order_points():
        words = ta.reference_comb(q, BITS, 2)
        assert not ta.flagged(ta.audit_flags(words, 2, ENTRIES)), q


@pytest.mark.parametrize("kind", [k for k in ta.MUTANTS if k != "previous_window"])
@pytest.mark.parametrize("w,j", [(0, 2), (1, 4), (2, ENTRIES - 2)])
def test_every_mutant_is_flagged_where_it_sits(comb, kind, w, j):
    _, words = comb
    bad, want = ta.mutate(words, kind, ENTRIES, w, j)
    assert (bad != words).any()
    assert ta.flagged(ta.audit_flags(bad, WINDOWS, ENTRIES)) == want
    assert set(want) <= {w * ENTRIES + j, w * ENTRIES + j + 1}


def test_value_preserving_mutants_keep_their_value(comb):
    """limb_plus_p and limb_carried_out leave every value alone (so only the bound bit may speak),
    and the exact check refuses them for the bound, not for the value."""
    point, words = comb
    pts = window_points(point, 1)
    for kind in ("limb_plus_p", "limb_carried_out"):
        bad, _ = ta.mutate(words, kind, ENTRIES, 1, 3)
        a, b = ta.entry_parts(words)[0], ta.entry_parts(bad)[0]
        assert all(((pp.values(a[:, k]) - pp.values(b[:, k])) % P == 0).all() for k in range(3))
        with pytest.raises(AssertionError, match="out of bound"):
            ta.check_entries(bad[ENTRIES:2 * ENTRIES], pts)


def test_a_window_of_the_wrong_point_passes_the_chain_and_fails_the_exact_check(comb):
    """Why both checks exist: a whole window replaced by the previous window's entries, or built from
    the wrong base, closes every chain; entries 0 and 1 against the reference give it away."""
    point, words = comb
    bad, want = ta.mutate(words, "previous_window", ENTRIES, 2, 0)
    assert want == {} and (bad[2 * ENTRIES:] == words[ENTRIES:2 * ENTRIES]).all()
    assert not ta.flagged(ta.audit_flags(bad, WINDOWS, ENTRIES))
    pts = window_points(point, 2)
    ta.check_entries(bad[2 * ENTRIES:2 * ENTRIES + 1], pts[:1], "entry 0 is the identity in any window")
    with pytest.raises(AssertionError, match="not the reference point"):
        ta.check_entries(bad[2 * ENTRIES:2 * ENTRIES + 2], pts[:2])
    # a builder that starts one bit late: window 1 holds multiples of 2^3 P instead of 2^4 P
    late = words.copy()
    late[ENTRIES:2 * ENTRIES] = [ta.niels_words(q) for q in ta.multiples(ref.pt_mul(1 << 3, point), 0, ENTRIES)]
    assert not ta.flagged(ta.audit_flags(late, WINDOWS, ENTRIES))
    with pytest.raises(AssertionError, match="not the reference point"):
        ta.check_entries(late[ENTRIES:ENTRIES + 2], window_points(point, 1)[:2])
    # entry 1 alone wrong: every later entry of the window breaks its chain
    one = words.copy()
    one[ENTRIES + 1] = words[ENTRIES + 2]
    assert set(ta.flagged(ta.audit_flags(one, WINDOWS, ENTRIES))) == set(range(ENTRIES + 2, 2 * ENTRIES))
    with pytest.raises(AssertionError, match="not the reference point"):
        ta.check_entries(one[ENTRIES:ENTRIES + 2], window_points(point, 1)[:2])
    # entry 0 not the identity
    zero = words.copy()
    zero[0] = words[3]
    assert ta.flagged(ta.audit_flags(zero, WINDOWS, ENTRIES)) == {0: ta.CHAIN, 1: ta.CHAIN}


def test_the_exact_check_rejects_each_kind_of_wrong_entry(comb):
    point, words = comb
    pts = window_points(point, 0)
    win = words[:ENTRIES]
    ta.check_entries(win, pts)
    for col, match in ((0, "ypx"), (10, "ymx"), (25, "xy2d")):
        bad = win.copy()
        bad[4, col] += 1
        with pytest.raises(AssertionError, match=match):
            ta.check_entries(bad, pts)
    bad = win.copy()
    bad[6, 30] = 7
    with pytest.raises(AssertionError, match="pad"):
        ta.check_entries(bad, pts)


def test_the_bound_bit_starts_one_past_the_class_maximum(comb):
    """A limb exactly at its class maximum is in bounds, one more is not: xy2d at tight, ypx and ymx
    at 2 x tight, either sign, even and odd limbs (the value moves, so other bits speak too)."""
    _, words = comb
    t = ENTRIES + 3
    for col, bound in ((20, pp.TIGHT[0]), (21, pp.TIGHT[1]), (0, 2 * pp.TIGHT[0]), (5, 2 * pp.TIGHT[1]),
                       (12, 2 * pp.TIGHT[0]), (19, 2 * pp.TIGHT[1])):
        for sign in (1, -1):
            edge = words.copy()
            lim = edge[:, :30].view(np.int32)
            lim[t, col] = sign * int(bound)
            assert not ta.audit_flags(edge, WINDOWS, ENTRIES)[t] & ta.BOUND
            lim[t, col] = sign * (int(bound) + 1)
            assert ta.audit_flags(edge, WINDOWS, ENTRIES)[t] & ta.BOUND


def test_key_flags_by_the_reference():
    rng = random.Random(5)
    honest = ref.pt_mul(rng.randrange(1, pp.L), ref.BASEPOINT)
    small = ref.small_order_points()
    assert ta.key_flags(ref.compress(honest)) == ta.KEY_DECODES
    assert ta.key_flags(ref.compress(ref.pt_add(honest, small[5]))) == ta.KEY_DECODES | ta.KEY_TORSION
    assert ta.key_flags(ref.compress(ref.IDENTITY)) == ta.KEY_DECODES | ta.KEY_SMALL_ORDER
    assert ta.key_flags(ref.compress(small[6])) == ta.KEY_DECODES | ta.KEY_SMALL_ORDER | ta.KEY_TORSION
    y = next(y for y in range(2, 100) if ref.decompress(y.to_bytes(32, "little")) is None)
    assert ta.key_flags(y.to_bytes(32, "little")) == 0
    # y = p + 1 = 1 mod p, sign bit set: dalek decodes it to the identity (x = -0)
    assert ta.key_flags((P + 1 + (1 << 255)).to_bytes(32, "little")) == ta.KEY_DECODES | ta.KEY_SMALL_ORDER
