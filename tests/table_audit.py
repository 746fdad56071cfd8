"""The host side of the table audit (tests/test_gpu_tables.py, tests/test_tables_host.py).

Every verification path adds entries of point tables the library builds once and keeps in device
memory.  An entry is an affine Niels point -- ypx = y + x, ymx = y - x, xy2d = 2 d x y as ten signed
limbs each, 120 bytes, or 128 with two zero pad words -- and entry j of a window claims to be
j * (the window's entry 1).  Three checks together prove every stored entry:

  * the exact check (check_entries): the stored limbs' values mod p against y + x, y - x, 2 d x y of
    the point oracle/ed25519_ref.py computes, the limb bounds the consumers assume and the pad words;
  * the audit (the probe's probe_table_audit on the device; audit_flags here is its restatement in
    Python integers): entry[j] = entry[j - 1] + entry[1] by the affine addition law, 2 xy2d = d X Y,
    bounds and pads, one flag word per entry;
  * induction: with entries 0 and 1 of a window exact, a window without a flag holds j * entry[1] at
    every j.

The exact check costs a scalar multiplication per sampled run, the audit a dozen field products per
entry, so the first is sampled (edges, powers of two, block and run boundaries, a random draw) and
the second covers everything.  Neither uses the library's group formulas.  mutate() makes the wrong
tables the checks must catch.
"""
from __future__ import annotations

import numpy as np

from oracle import ed25519_ref as ref
from tests import prim_probe as pp

P = pp.P
CHAIN, NIELS, BOUND, PAD = pp.AUDIT_CHAIN, pp.AUDIT_NIELS, pp.AUDIT_BOUND, pp.AUDIT_PAD
IDENTITY = (0, 1)

# flags of nwc_set_committee's, the auto cache's and the launch keys' key arrays (kernels.hip)
KEY_DECODES, KEY_SMALL_ORDER, KEY_TORSION = 1, 2, 4


# ---- reference generators ---------------------------------------------------------------------
def multiples(point, first: int, count: int):
    """[first * point, (first + 1) * point, ...]: one pt_mul, then one pt_add per entry."""
    out = [ref.pt_mul(first, point)]
    for _ in range(count - 1):
        out.append(ref.pt_add(out[-1], point))
    return out


def window_base(point, bits: int, w: int):
    """2^(bits w) * point: entry 1 of window w of a radix-2^bits comb."""
    return ref.pt_mul(1 << (bits * w), point)


def niels_values(point):
    x, y = point
    return ((y + x) % P, (y - x) % P, 2 * ref.D * x * y % P)


def niels_words(point, pad=(0, 0)) -> np.ndarray:
    """An entry as the builders store it: ypx, ymx as limb-wise sum and difference of the tight limbs
    of y and x, xy2d tight, the pad words: 32 uint32 words."""
    x, y = point
    cx, cy = np.array(pp.centred_limbs(x)), np.array(pp.centred_limbs(y))
    limbs = np.concatenate([cy + cx, cy - cx, pp.centred_limbs(2 * ref.D * x * y), pad])
    return limbs.astype(np.int64).astype(np.int32).view(np.uint32)


def reference_comb(point, bits: int, windows: int) -> np.ndarray:
    """comb[w * E + j] = j * 2^(bits w) * point, E = 2^(bits - 1) + 1: (windows * E, 32) words."""
    entries = (1 << (bits - 1)) + 1
    rows = []
    for w in range(windows):
        rows += [niels_words(q) for q in multiples(window_base(point, bits, w), 0, entries)]
    return np.array(rows, dtype=np.uint32)


def key_flags(key: bytes) -> int:
    """KEY_DECODES | KEY_SMALL_ORDER | KEY_TORSION of a 32-byte key, by the reference: the small-order
    bit goes by the canonical y alone (it is set for an encoding of such a y that does not decode)."""
    a = ref.decompress(key)
    y = (int.from_bytes(key, "little") & ((1 << 255) - 1)) % P
    small = y in {pt[1] for pt in ref.small_order_points()}
    return (KEY_DECODES if a is not None else 0) | (KEY_SMALL_ORDER if small else 0) | \
        (KEY_TORSION if a is not None and ref.has_torsion(a) else 0)


# ---- the exact check --------------------------------------------------------------------------
def entry_parts(words: np.ndarray):
    """(n, 32) words -> signed limbs (n, 3, 10), pad words (n, 2)."""
    words = np.asarray(words, dtype=np.uint32)
    assert words.ndim == 2 and words.shape[1] == 32, words.shape
    return pp.signed(words[:, :30]).reshape(-1, 3, 10), words[:, 30:]


ENTRY_BOUNDS = np.stack([2 * pp.TIGHT, 2 * pp.TIGHT, pp.TIGHT])     # ypx, ymx <= 2 x tight; xy2d <= tight


def check_entries(words: np.ndarray, points, what: str = "") -> None:
    """Stored entries against reference points: values mod p exactly, limbs within the classes the
    consumers assume (prim_probe.SIGNED_CLASSES "2T", "2T", "T"), pad words zero."""
    limbs, pad = entry_parts(words)
    assert len(limbs) == len(points), (what, len(limbs), len(points))
    for k, name in enumerate(("ypx", "ymx", "xy2d")):
        got = pp.values(limbs[:, k, :])
        want = np.array([niels_values(q)[k] for q in points], dtype=object)
        bad = (got - want) % P != 0
        assert not bad.any(), "%s: %s is not the reference point's at entries %s" % (what, name, pp._first(bad))
    over = (np.abs(limbs) > ENTRY_BOUNDS).any(axis=(1, 2))
    assert not over.any(), "%s: limb out of bound at entries %s" % (what, pp._first(over))
    dirty = (pad != 0).any(axis=1)
    assert not dirty.any(), "%s: pad words set at entries %s" % (what, pp._first(dirty))


# ---- the audit, restated ----------------------------------------------------------------------
def audit_flags(words: np.ndarray, windows: int, entries: int, one_offset: int = 1, one_stride: int = None) -> np.ndarray:
    """probe_table_audit in Python integers: one flag word per entry of windows x entries entries."""
    one_stride = entries if one_stride is None else one_stride
    limbs, pad = entry_parts(words)
    assert len(limbs) >= windows * entries
    val = [[int(v) % P for v in pp.values(limbs[:, k, :])] for k in range(3)]
    flags = np.zeros(windows * entries, dtype=np.uint32)
    over = (np.abs(limbs) > ENTRY_BOUNDS).any(axis=(1, 2))
    dirty = (pad != 0).any(axis=1)
    d = ref.D
    for t in range(windows * entries):
        w, j = divmod(t, entries)
        f = (BOUND if over[t] else 0) | (PAD if dirty[t] else 0)
        x3, y3 = (val[0][t] - val[1][t]) % P, (val[0][t] + val[1][t]) % P        # 2x, 2y
        if (2 * val[2][t] - d * x3 * y3) % P:
            f |= NIELS
        if j == 0:
            if val[0][t] != 1 or val[1][t] != 1:
                f |= CHAIN
        else:
            o = one_offset + w * one_stride
            x1, y1 = (val[0][t - 1] - val[1][t - 1]) % P, (val[0][t - 1] + val[1][t - 1]) % P
            x2, y2 = (val[0][o] - val[1][o]) % P, (val[0][o] + val[1][o]) % P
            m = d * x1 * x2 * y1 * y2 % P
            if (x3 * (16 + m) - 8 * (x1 * y2 + y1 * x2)) % P or (y3 * (16 - m) - 8 * (y1 * y2 + x1 * x2)) % P:
                f |= CHAIN
        flags[t] = f
    return flags


def flagged(flags: np.ndarray) -> dict:
    """{index: flag word} of the flagged entries."""
    return {int(i): int(flags[i]) for i in np.nonzero(flags)[0]}


# ---- mutants ----------------------------------------------------------------------------------
P_LIMBS = np.array(pp.limbs_of(P), dtype=np.int64)                  # p's own limbs: 2^26 - 19, 2^25 - 1, ...

MUTANTS = ("xy2d_plus_one", "next_entry", "negated", "limb_plus_p", "limb_carried_out", "pad_set", "previous_window")


def mutate(words: np.ndarray, kind: str, entries: int, w: int, j: int):
    """A copy of a table with one defect at entry j of window w, and what the audit must say:
    (mutant words, {index: flag word}).  2 <= j <= entries - 2, so the entry has a successor in its
    window and is not the window's entry 1 (whose defects only the exact check can see, as every
    entry of the window is then a multiple of the wrong point)."""
    out = np.array(words, dtype=np.uint32, copy=True)
    lim = out[:, :30].view(np.int32)
    t = w * entries + j
    assert 2 <= j <= entries - 2 or kind == "previous_window"
    if kind == "xy2d_plus_one":          # one limb of xy2d + 1: x and y untouched, so the chain holds
        lim[t, 20 + 3] += 1
        return out, {t: NIELS}
    if kind == "next_entry":             # a valid point in the wrong place: (j + 1) P at j
        out[t] = out[t + 1]
        return out, {t: CHAIN, t + 1: CHAIN}
    if kind == "negated":                # -(x, y) = (-x, y): ypx <-> ymx, -xy2d
        lim[t, 0:10], lim[t, 10:20] = lim[t, 10:20].copy(), lim[t, 0:10].copy()
        lim[t, 20:30] = -lim[t, 20:30]
        return out, {t: CHAIN, t + 1: CHAIN}
    if kind == "limb_plus_p":            # the same value: xy2d + p limb by limb, every limb a width up
        lim[t, 20:30] += P_LIMBS.astype(np.int32)
        return out, {t: BOUND}
    if kind == "limb_carried_out":       # the same value: 3 units of ypx's limb 4 moved down into limb 3 (3 x 2^25 there,
        lim[t, 3] += 3 << 25             # past 2 x tight whatever the limb held)
        lim[t, 4] -= 3
        return out, {t: BOUND}
    if kind == "pad_set":
        out[t, 31] = 1
        return out, {t: PAD}
    if kind == "previous_window":        # window w holds window w - 1's entries: every chain still closes
        assert w >= 1
        out[w * entries:(w + 1) * entries] = out[(w - 1) * entries:w * entries]
        return out, {}
    raise ValueError(kind)


# ---- the device's tables (the GPU tests and their subprocess helper) -------------------------
KEY_BITS, KEY_WINDOWS = 14, 19
KEY_ENTRIES = (1 << (KEY_BITS - 1)) + 1
COMB_RUN = 8                                                    # kernels.hip: entries a lane builds per inversion


def doublings(point, count: int):
    """[point, 2 point, 4 point, ...], count + 1 of them."""
    out = [point]
    for _ in range(count):
        out.append(ref.pt_add(out[-1], out[-1]))
    return out


def window_samples(pw, entries: int, runs=(), neighbours: bool = True) -> dict:
    """{j: j * base} of one window with entries = 2^(bits - 1) + 1 from pw = doublings(base, bits - 1):
    0, 1, 2, entries - 2, entries - 1, with `neighbours` 2^k - 1, 2^k, 2^k + 1 for every k, and the
    runs (first j, count) of consecutive entries: one pt_mul and count - 1 pt_add each."""
    base, top = pw[0], len(pw) - 1
    assert entries == (1 << top) + 1
    out = {0: IDENTITY, 1: base, 2: pw[1], entries - 1: pw[top], entries - 2: ref.pt_add(pw[top], ref.pt_neg(base))}
    if neighbours:
        for k in range(1, top + 1):
            out[1 << k] = pw[k]
            out[(1 << k) - 1] = ref.pt_add(pw[k], ref.pt_neg(base))
            if k < top:
                out[(1 << k) + 1] = ref.pt_add(pw[k], base)
    for first, count in runs:
        assert 0 <= first and first + count <= entries
        for i, q in enumerate(multiples(base, first, count)):
            out[first + i] = q
    return out


def check_window(table, first: int, samples: dict, what: str) -> None:
    """The sampled entries {j: point} of the window that starts at element `first`, exactly."""
    js = sorted(samples)
    check_entries(pp.gather(table, [first + j for j in js]), [samples[j] for j in js], what)


def clean(table, windows: int, entries: int, what: str, skip=()) -> None:
    """The audit over windows x entries entries leaves no flag (outside the windows in `skip`)."""
    idx, flags = pp.audit_table(table, windows, entries)
    keep = ~np.isin(idx // entries, list(skip))
    assert not keep.any(), "%s: the audit flags %d entries, the first at (window, entry, flags) %s" % (
        what, int(keep.sum()), [(int(i) // entries, int(i) % entries, int(f)) for i, f in zip(idx[keep][:6], flags[keep][:6])])


def check_key_arrays(owner: str, expect_keys, rng, tables: bool = True):
    """The per-key arrays of one owner ("committee", "auto", "launch") against the keys it should
    hold, in order: the key bytes and the flags bit for bit; for every key that decodes the
    129-entry table (entry j = j (-A)) exactly, the audit over all 19 x 8,193 comb entries, and
    exactly: entries 0, 1, 2, 8,191, 8,192 of every window (entry 1 = 2^(14 w) (-A); 8,192 is the
    builder's one-entry last run) and a random pair of neighbours in every window; in two windows per
    key (rotating with the key's index) also the neighbours of every power of two and a whole sampled
    run with the entries either side of it (j = 7, 8 mod 8).  Prints what it covered."""
    n = len(expect_keys)
    keys_arr, held = pp.library_table(owner + "_keys")
    assert held == n, (owner, held, n)
    got = pp.read_array(keys_arr).astype("<u4")
    assert [got[i].tobytes() for i in range(n)] == [bytes(k) for k in expect_keys], owner + ": keys"
    flags_arr, held_f = pp.library_table(owner + "_flags")
    assert held_f == n
    want_flags = [key_flags(bytes(k)) for k in expect_keys]
    assert pp.read_array(flags_arr).reshape(-1).tolist() == want_flags, owner + ": flags"
    decoded = [i for i in range(n) if want_flags[i] & KEY_DECODES]
    bases = {i: ref.pt_neg(ref.decompress(bytes(expect_keys[i]))) for i in decoded}
    bad_keys = [i for i in range(n) if i not in bases]
    if tables:
        tab, held_t = pp.library_table(owner + "_tables")
        assert held_t == n and tab.stride == 120 and tab.elements == n * 129
        clean(tab, n, 129, owner + " tables", skip=bad_keys)
        for i in decoded:
            check_entries(pp.gather(tab, np.arange(129) + 129 * i), multiples(bases[i], 0, 129), "%s table of key %d" % (owner, i))
    comb, held_c = pp.library_table(owner + "_comb")
    assert held_c == n and comb.stride == 128 and comb.elements == n * KEY_WINDOWS * KEY_ENTRIES
    clean(comb, n * KEY_WINDOWS, KEY_ENTRIES, owner + " comb",
          skip=[i * KEY_WINDOWS + w for i in bad_keys for w in range(KEY_WINDOWS)])
    exact = 0
    for i in decoded:
        pw = doublings(bases[i], KEY_BITS * KEY_WINDOWS)
        full = {(i + 7 * k) % KEY_WINDOWS for k in range(2)}
        for w in range(KEY_WINDOWS):
            runs = [(rng.randrange(3, KEY_ENTRIES - 4), 2)]     # every window: a random pair of neighbours
            if w in full:
                r = rng.randrange(1, (KEY_ENTRIES - 1) // COMB_RUN)
                runs.append((COMB_RUN * r - 1, COMB_RUN + 2))
            samples = window_samples(pw[KEY_BITS * w:KEY_BITS * w + KEY_BITS], KEY_ENTRIES, runs, neighbours=w in full)
            check_window(comb, (i * KEY_WINDOWS + w) * KEY_ENTRIES, samples, "%s comb of key %d, window %d" % (owner, i, w))
            exact += len(samples)
    print("%s: %d keys (%d decode); %d comb entries audited; %d comb entries exact: ends and a random pair in every window, "
          "powers of two and a whole run with its neighbours in 2 of the 19 windows per key%s" % (
              owner, n, len(decoded), n * KEY_WINDOWS * KEY_ENTRIES, exact,
              "; %d table entries exact" % (129 * len(decoded)) if tables else ""))
    return want_flags
