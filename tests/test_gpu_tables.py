"""Every stored entry of every precomputed point table is the point it claims to be.

Every verification path adds entries of tables the library builds once and keeps in device memory:
the basepoint tables (base_table, sign_table, comb_base, the 2.1 GB base24, the 3.2 GB comb16) and,
per key, a 129-entry ladder table and a 19 x 8,193-entry comb in three owners (the committee, the
auto key cache, the launch keys).  The other tests judge them by one bit per signature, and a given
base24 entry is read less than once in a million verifications.  Here nwc_diag_table says where a
table lives, and the probe library (tests/hip/prim_probe.hip) reads it:

  * the small tables entry by entry against oracle/ed25519_ref.py;
  * the large ones by the audit -- every entry is the previous one plus the window's entry 1, by the
    affine addition law written out on the stored values, with the Niels product, the limb bounds and
    the pad words -- plus the exact check of entries 0 and 1 of every window, which together prove a
    window by induction, and exact samples where a builder could slip: the ends of a window, the
    neighbours of every power of two, block and run boundaries, a random draw.

Nothing takes a tolerance: values are compared mod p, flags and keys bit for bit.  The audit must
be able to fail: the mutants of tests/table_audit.py, applied to copies of real tables, are flagged at
exactly the expected entries.  Checks, reference generators and mutants live in tests/table_audit.py
(tested without a device by tests/test_tables_host.py).
"""
import ctypes
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import prim_probe as pp
from tests import table_audit as ta
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

P, L = pp.P, pp.L
B = ref.BASEPOINT
HELPER = os.path.join(ROOT, "tests", "table_audit_helper.py")


@pytest.fixture(scope="module")
def lib():
    """The library with its basepoint tables built: one small verify call and one signer."""
    pp.load()
    from narwhal_amd import _lib
    lib = _lib.load()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verify.json")))
    ok = next(c for c in gold["cases"] if c["name"] == "ref-verify_valid_signature")
    m, k, s = (bytes.fromhex(ok[f]) for f in ("msg", "pk", "sig"))
    assert lib.nwc_verify_strict(_lib.buf(m), _lib.buf(k), _lib.buf(s)) == 0
    pair = ctypes.create_string_buffer(64)
    _lib.check(lib.nwc_keypair_from_seed(_lib.buf(bytes(range(32))), pair))
    signer = lib.nwc_signer_create(_lib.buf(pair.raw))
    assert signer
    _lib.check(lib.nwc_signer_destroy(signer))
    return lib


def timed(what, t0):
    print("%s: %.2f s" % (what, time.time() - t0))


# ---- basepoint tables -------------------------------------------------------------------------
def test_small_basepoint_tables_entry_by_entry(lib):
    """base_table (j B and j 2^132 B, j = 0..128), sign_table (j 16^w B, j = 1..8, 64 windows) and
    comb_base (j 256^w B, j = 0..128, 32 windows): every entry against the reference, each window
    walked by one pt_add per entry; and the audit over the two tables that have an entry 0."""
    t0 = time.time()
    tab, _ = pp.library_table("base_table")
    assert (tab.stride, tab.elements) == (120, 258)
    want = ta.multiples(B, 0, 129) + ta.multiples(ref.pt_mul(1 << 132, B), 0, 129)
    ta.check_entries(pp.gather(tab, np.arange(258)), want, "base_table")
    ta.clean(tab, 2, 129, "base_table")
    tab, _ = pp.library_table("sign_table")
    assert (tab.stride, tab.elements) == (120, 512)
    want, base = [], B
    for w in range(64):
        want += ta.multiples(base, 1, 8)
        base = ta.doublings(base, 4)[-1]
    ta.check_entries(pp.gather(tab, np.arange(512)), want, "sign_table")
    tab, _ = pp.library_table("comb_base")
    assert (tab.stride, tab.elements) == (128, 32 * 129)
    want, base = [], B
    for w in range(32):
        want += ta.multiples(base, 0, 129)
        base = ta.doublings(base, 8)[-1]
    ta.check_entries(pp.gather(tab, np.arange(32 * 129)), want, "comb_base")
    ta.clean(tab, 32, 129, "comb_base")
    print("small basepoint tables: %d entries exact" % (258 + 512 + 32 * 129))
    timed("test_small_basepoint_tables_entry_by_entry", t0)


def large_table(name, windows, bits, bases, rng, runs_per_window, block_cuts):
    """A large basepoint table: the audit over every entry, and per window exactly: entries 0, 1, 2,
    E - 2, E - 1, the neighbours of every power of two, the two entries either side of `block_cuts`
    boundaries of the builder's 256-lane blocks (element index = 0 mod 256), and `runs_per_window`
    random runs of four consecutive entries."""
    tab, _ = pp.library_table(name)
    entries = (1 << (bits - 1)) + 1
    assert tab is not None and (tab.stride, tab.elements) == (128, windows * entries), name
    ta.clean(tab, windows, entries, name)
    exact = 0
    for w in range(windows):
        runs = [(rng.randrange(3, entries - 6), 4) for _ in range(runs_per_window)]
        first = w * entries
        for _ in range(block_cuts):                             # j with (first + j) a multiple of 256
            cut = rng.randrange((first + 2) // 256 + 1, (first + entries - 2) // 256) * 256
            runs.append((cut - first - 1, 2))
        samples = ta.window_samples(ta.doublings(bases[w], bits - 1), entries, runs)
        ta.check_window(tab, first, samples, "%s window %d" % (name, w))
        exact += len(samples)
    return tab, entries, exact


def test_base24_every_entry(lib):
    """base24[h (2^23 + 1) + j] = j 2^(141 h) B.  The halves' boundary -- the last entry of the first
    half (digit 2^23, read once in about 1.5 million verifications) and entries 0 and 1 of the second
    -- is among the exact entries, like B and 2^141 B themselves."""
    t0 = time.time()
    rng = random.Random(2401)
    bases = [B, ref.pt_mul(1 << 141, B)]
    tab, entries, exact = large_table("base24", 2, 24, bases, rng, runs_per_window=16, block_cuts=6)
    ta.check_entries(pp.gather(tab, [entries - 1, entries, entries + 1, 2 * entries - 1]),
                     [ref.pt_mul(1 << 23, B), ta.IDENTITY, bases[1], ref.pt_mul(1 << 164, B)], "base24 halves")
    print("base24: %d entries audited, %d exact" % (2 * entries, exact + 4))
    timed("test_base24_every_entry", t0)


def test_comb16_every_entry(lib):
    """comb16[w (2^21 + 1) + j] = j 2^(22 w) B, 12 windows."""
    t0 = time.time()
    rng = random.Random(2201)
    bases = ta.doublings(B, 22 * 11)[::22]
    assert len(bases) == 12 and bases[3] == ref.pt_mul(1 << 66, B)
    tab, entries, exact = large_table("comb16", 12, 22, bases, rng, runs_per_window=6, block_cuts=3)
    print("comb16: %d entries audited, %d exact" % (12 * entries, exact))
    timed("test_comb16_every_entry", t0)


def run_helper(mode, tmp_path, env=None, timeout=600):
    out = tmp_path / (mode + ".json")
    t0 = time.time()
    r = subprocess.run([sys.executable, HELPER, ROOT, mode, str(out)], env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    timed("helper %s" % mode, t0)
    return json.load(open(out))


def test_without_comb16_the_rest_still_passes(tmp_path):
    """NWC_COMB16=0: comb16 reports address 0, the other basepoint tables are audited as before."""
    log = run_helper("nocomb16", tmp_path, {"NWC_COMB16": "0"})
    assert log["comb16"] is None
    assert log["audited"] == {"base_table": 258, "comb_base": 32 * 129, "base24": 2 * ((1 << 23) + 1)}
    assert log["exact"] >= 258 + 8


# ---- committee --------------------------------------------------------------------------------
def committee_keys():
    """Honest keys, a key with a torsion component, the small-order points in canonical and in the
    non-canonical encodings that decode, a non-canonical y >= p off the small-order set, and a key
    that does not decode."""
    rng = random.Random(77)
    small = ref.small_order_points()
    honest = [ref.pt_mul(rng.randrange(1, L), B) for _ in range(4)]
    top = 1 << 255
    enc = lambda v: int(v).to_bytes(32, "little")   # noqa: E731
    keys = [ref.compress(q) for q in honest[:3]]
    keys.append(ref.compress(ref.pt_add(honest[3], small[4])))              # honest + a point of order 8
    keys += [ref.compress(small[0]), ref.compress(small[1]), ref.compress(small[2]), ref.compress(small[5])]
    keys += [enc(1 | top), enc(P), enc(P | top), enc((P + 1) | top), enc((P - 1) | top)]   # x = -0; y = p, p + 1 as 0, 1
    k = next(k for k in range(2, 19) if ref.decompress(enc(P + k)) is not None)
    keys.append(enc(P + k))                                                 # y >= p, decodes, not small order
    y = next(y for y in range(2, 100) if ref.decompress(enc(y)) is None)
    keys.append(enc(y))
    assert len(set(keys)) == len(keys) == 15
    flags = [ta.key_flags(k) for k in keys]
    assert flags[:4] == [1, 1, 1, 5] and flags[-1] == 0 and flags[-2] & 1 and not flags[-2] & 2
    assert all(f & 3 == 3 for f in flags[4:13])
    return keys


def test_committee_tables_and_combs(lib):
    """nwc_set_committee takes every key (it never judges them); committee_keys are the keys given, in
    order, committee_flags the reference's decodes / small order / torsion, and for every key that
    decodes the 129-entry table and the comb are that key's (table_audit.check_key_arrays).  For the
    key that does not decode only the flags are checked."""
    from narwhal_amd import _lib
    t0 = time.time()
    keys = committee_keys()
    _lib.check(lib.nwc_set_committee(_lib.buf(b"".join(keys)), len(keys)))
    try:
        flags = ta.check_key_arrays("committee", keys, random.Random(1401))
        assert flags[-1] == 0
    finally:
        _lib.check(lib.nwc_set_committee(None, 0))
    for name in ("committee_keys", "committee_flags", "committee_tables", "committee_comb"):
        assert pp.library_table(name) == (None, 0), name
    print("committee: %d keys, %d comb entries audited" % (len(keys), len(keys) * 19 * 8193))
    timed("test_committee_tables_and_combs", t0)


def test_auto_key_cache_after_regrow_and_wrap(tmp_path):
    """NWC_AUTO_KEYS=20: 24 keys seen twice each through two-key certificates.  The cache regrows once
    (16 -> 20 keys, stream-ordered copies) and the last four keys replace the oldest four, so it holds
    keys 20..23, 4..19 in that order; every held key's flags, table and comb are its own, and a last
    round of certificates (one vote in three corrupted) gets the oracle's verdicts."""
    log = run_helper("auto", tmp_path, {"NWC_AUTO_KEYS": "20"})
    assert log["held"] == list(range(20, 24)) + list(range(4, 20))
    assert log["capacity"] == 20 and log["checked_keys"] == 20
    assert log["verdicts"] == log["oracle"] and 0 < sum(r for r, _ in log["verdicts"]) < len(log["verdicts"])


def test_launch_keys_after_each_launch(tmp_path):
    """Batch-leaf launches of 65,536 equations without a committee: 6 repeated keys join at the first
    (room for 8), 2 of 6 further keys at the second, and the third grows the comb buffer behind the
    held combs (8 -> 16) for the rest.  After each launch the held keys, their flags and their combs
    pass the committee's checks; the first keys keep their places through the growth."""
    log = run_helper("launch", tmp_path)
    assert [e["held"] for e in log["launches"]] == [6, 8, 12]
    for e in log["launches"]:
        assert e["verdicts_ok"] and e["checked_keys"] == e["held"]
    assert log["launches"][1]["keys"][:6] == log["launches"][0]["keys"]
    assert log["launches"][2]["keys"][:8] == log["launches"][1]["keys"]
    assert sorted(log["launches"][2]["keys"]) == sorted(log["expected_keys"])


# ---- the audit must be able to fail -----------------------------------------------------------
@pytest.fixture(scope="module")
def copies(lib):
    """Test-owned copies of comb_base (32 x 129) and of three windows of a key comb (3 x 8,193)."""
    from narwhal_amd import _lib
    tab, _ = pp.library_table("comb_base")
    base = pp.gather(tab, np.arange(32 * 129))
    key = ref.compress(ref.pt_mul(987654321, B))
    _lib.check(lib.nwc_set_committee(_lib.buf(key), 1))
    try:
        comb, _ = pp.library_table("committee_comb")
        win = pp.gather(comb, np.arange(3 * ta.KEY_ENTRIES) + 4 * ta.KEY_ENTRIES)     # windows 4, 5, 6
    finally:
        _lib.check(lib.nwc_set_committee(None, 0))
    return {"comb_base": (base, 32, 129, ref.pt_mul(1 << 8, B)),
            "key comb": (win, 3, ta.KEY_ENTRIES, ref.pt_neg(ref.pt_mul(987654321 << (14 * 5), B)))}


def device_flags(words, windows, entries):
    idx, flags = pp.audit_table(pp.device_copy(words), windows, entries)
    return {int(i): int(f) for i, f in zip(idx, flags)}


@pytest.mark.parametrize("which", ["comb_base", "key comb"])
def test_mutants_of_real_tables_are_flagged(copies, which):
    """Each mutant of a copy of a real table is flagged at exactly the expected entries with the
    expected bit -- the mutated entry and, where the value moved, its successor -- also at the ends of a
    window, at a run boundary of the key comb's builder, and in the last entry's neighbourhood; the
    untouched copy has no flag.  A window replaced by the previous window's entries is missed by the
    chain and caught by the exact check of its entry 1."""
    t0 = time.time()
    words, windows, entries, base_of_window_1 = copies[which]
    assert device_flags(words, windows, entries) == {}
    spots = [(0, 2), (1, 7), (1, 8), (windows - 1, entries - 2), (1, entries // 2)]
    caught = 0
    for kind in ta.MUTANTS:
        if kind == "previous_window":
            continue
        for w, j in spots:
            bad, want = ta.mutate(words, kind, entries, w, j)
            assert want and device_flags(bad, windows, entries) == want, (which, kind, w, j)
            caught += 1
    assert caught == 6 * len(spots)
    print("%s: %d mutants of %d entries, each flagged at exactly the expected entries" % (which, caught, len(words)))
    bad, want = ta.mutate(words, "previous_window", entries, 1, 0)
    assert want == {} and device_flags(bad, windows, entries) == {}
    good = [ta.IDENTITY, base_of_window_1]
    ta.check_entries(words[entries:entries + 2], good, which)
    with pytest.raises(AssertionError, match="not the reference point"):
        ta.check_entries(bad[entries:entries + 2], good, which)
    # the restated audit (tests/test_tables_host.py) and the kernel agree on a mutant with every bit set somewhere
    mixed = words[:2 * entries].copy()
    for kind, j in (("xy2d_plus_one", 3), ("negated", 9), ("limb_plus_p", 20), ("pad_set", 30), ("next_entry", entries + 5)):
        mixed, _ = ta.mutate(mixed, kind, entries, j // entries, j % entries)
    both = ta.flagged(ta.audit_flags(mixed, 2, entries))
    assert len(both) == 7 and device_flags(mixed, 2, entries) == both
    timed("test_mutants_of_real_tables_are_flagged[%s]" % which, t0)
