"""GPU tests of the layer between the primitives and the verdicts: the half-size scalars, the digit
strings and the two half-size ladders at every width of (c, d) the kernels accept.

Every verify kernel rewrites s B - k A - R = O as (d s mod l) B - c A - d R = O with (c, d) =
lat::reduce(k) (narwhal_amd/csrc/lattice.h).  tests/test_lattice_host.py checks the host build of that
header only, natural challenges stop at 132-133 bits (tests/test_gpu_wide.py), and the forced window
counts there carry zero digits in the top windows.  Here the half-size probe
(tests/hip/half_probe.hip, built by __graft_entry__.build() with the library's flags) runs each piece
alone on the device and compares it exactly with the integer models of tests/half_model.py: nothing
here takes a tolerance.

  * lat::reduce on 23,020 ordinary k and 1,280 constructed k (every bit length of max(|c|, d) from 128
    to 146 at least 16 times, ok clear at least 64 times): the four properties, bits, the sign flag,
    Euclid's row where the stopping cofactor is odd, and the host build lane for lane.  Borderline
    records of the even-cofactor branch's estimate of m (device and host one apart, both sound): 0
    expected; the count measured is in DESIGN.md section 2.4.
  * challenge<false> and challenge<true> against hashlib.
  * ds_mod_l, base_digits and the parked words as base_fetch reads them.
  * recode16 / recode256 / geu_recode4 for every W in 33..37 and every joint W in 66..74, drained every
    way the kernels drain them.
  * wave_windows / wave_windows4 against the integer formula.
  * half_scalarmult and half_scalarmult_cached on keys and nonces with known discrete logarithms, s
    chosen so that the result is t B for t in {0, 0, 1, 2, l - 1, 7}.
"""
import hashlib
import json
import os
import random
import subprocess
import time

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import half_model as hm
from tests import half_probe as hp
from tests import prim_probe as pp
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

P, L = hm.P, hm.L


@pytest.fixture(scope="module", autouse=True)
def probe():
    return hp.load()        # a missing or stale probe library is an error, not a skip


def report(family, records, extra=""):
    print("%s: %d records%s" % (family, records, extra))


# ---- lat::reduce ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lat():
    return hm.host_lattice()


def check_reduce_set(host_lat, ks, what):
    """One record set through probe_lat_reduce (whole and ragged) and every assertion of the module's
    docstring; returns (widths, oks, borderline count)."""
    rec = hp.ragged(hp.to_words(ks, 8))
    ks = ks + ks[:len(rec) - len(ks)]
    out = hp.run_whole_and_ragged("probe_lat_reduce", rec)
    cs, ds = hp.words_value(out[:, 0:5]), hp.words_value(out[:, 5:10])
    borderline, widths, oks = 0, [], []
    for i, k in enumerate(ks):
        c_abs, d, c_neg, ok, bits = cs[i], ds[i], int(out[i, 10]), int(out[i, 11]), int(out[i, 12])
        tag = "%s record %d" % (what, i)
        assert c_neg in (0, 1) and ok in (0, 1), tag
        hm.check_half_scalars(k, c_abs, d, c_neg, ok, bits, tag)
        if ok:
            hm.check_against_model(k, c_abs, d, c_neg, tag)
        hc, hd, hneg, hok = hm.host_reduce(host_lat, k)
        assert ok == hok, "%s: ok %d, the host build says %d, k = %d" % (tag, ok, hok, k)
        if (c_abs, d, c_neg) != (hc, hd, hneg):
            # only a borderline of the even-cofactor branch's double-precision estimate of m is allowed
            hm.check_half_scalars(k, hc, hd, hneg, hok, max(hc.bit_length(), hd.bit_length()), tag + " (host)")
            m_dev, m_host = hm.even_branch_m(k, c_abs, d, c_neg), hm.even_branch_m(k, hc, hd, hneg)
            assert hm.euclid(k)[1][1] % 2 == 0 and m_dev is not None and m_host is not None, \
                "%s: differs from the host build outside the even-cofactor branch, k = %d" % (tag, k)
            assert abs(m_dev - m_host) <= 1, "%s: m = %d, the host's %d, k = %d" % (tag, m_dev, m_host, k)
            assert abs(bits - max(hc.bit_length(), hd.bit_length())) <= 1, tag
            borderline += 1
        widths.append(bits)
        oks.append(ok)
    return widths, oks, borderline


def test_lat_reduce_ordinary(host_lat):
    """20,000 random k, 3,000 near-rational k, the edge list: device = host, the properties hold."""
    t0 = time.time()
    ks = hm.ordinary_k()
    widths, oks, borderline = check_reduce_set(host_lat, ks, "ordinary")
    assert all(oks[:20000])        # the random k all reduce (tests/test_lattice_host.py: test_random_k, the same seed)
    report("lat::reduce ordinary", len(ks), ", %d with ok clear, widest %d bits, %d borderline; %.1f s" % (
        len(oks) - sum(oks), max(w for w, ok in zip(widths, oks) if ok), borderline, time.time() - t0))
    assert borderline == 0


def test_lat_reduce_constructed(host_lat):
    """1,280 k whose Euclid sequence stops on an even cofactor of 96..127 bits: max(|c|, d) of every bit
    length 128..146 (at least 16 records each by the host build, asserted before the launch) and at
    least 64 records past 146 bits, which must report ok = 0."""
    t0 = time.time()
    ks = hm.constructed_k(seed=2146)
    host = [hm.host_reduce(host_lat, k) for k in ks]
    hm.check_population([max(h[0].bit_length(), h[1].bit_length()) for h in host], [h[3] for h in host])
    widths, oks, borderline = check_reduce_set(host_lat, ks, "constructed")
    per, failed = hm.class_counts(widths[:len(ks)], oks[:len(ks)])
    hm.check_population(widths[:len(ks)], oks[:len(ks)])
    report("lat::reduce constructed", len(ks), ", ok per width %s, %d with ok clear, %d borderline; %.1f s" % (
        sorted(per.items()), failed, borderline, time.time() - t0))
    assert borderline == 0


# ---- challenge --------------------------------------------------------------------------------
def test_challenge_both_variants():
    """k = SHA-512(R || A || M) mod l on 4,096 random triples and the golden cases with 32-byte messages."""
    rng = random.Random(64)
    rows = [rng.getrandbits(768).to_bytes(96, "little") for _ in range(4096)]
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verify.json")))
    n_gold = 0
    for c in gold["cases"]:
        m, k, s = (bytes.fromhex(c[f]) for f in ("msg", "pk", "sig"))
        if len(m) == 32 and len(k) == 32 and len(s) == 64:
            rows.append(s[:32] + k + m)
            n_gold += 1
    assert n_gold > 0
    rows += [bytes(96), b"\xff" * 96]
    rec = hp.ragged(np.frombuffer(b"".join(rows), dtype="<u4").reshape(-1, 24).astype(np.uint32))
    out = hp.run_whole_and_ragged("probe_challenge", rec)
    want = [int.from_bytes(hashlib.sha512(r.astype("<u4").tobytes()).digest(), "little") % L for r in rec]
    assert hp.words_value(out[:, :8]) == want, "challenge<false>"
    assert hp.words_value(out[:, 8:]) == want, "challenge<true>"
    report("challenge", len(rec), " (%d golden)" % n_gold)


# ---- base_digits ------------------------------------------------------------------------------
def check_base_output(out, rows, what):
    eb = hp.words_value(out[:, :8])
    dig = hp.signed(out[:, 8:31])
    for i, (d, s) in enumerate(rows):
        tag = "%s row %d" % (what, i)
        hm.check_base_digits(eb[i], dig[i, 0:6], dig[i, 6:11], d, s, tag)
        assert (dig[i, 11:22] == dig[i, 0:11]).all(), "%s: base_fetch reads other digits than base_digits made" % tag
        assert dig[i, 22] == 11, tag


def test_base_digits():
    """ds_mod_l, the split at 2^141, recode24<6> / recode24<5> and the parked layout: about 4,000 random
    (d, s) over every width of d and the edge rows (e = d s mod l chosen, s solved for)."""
    edges = hm.base_digit_edges(seed=24)
    rows = edges + hm.random_base_rows(seed=25)
    rec = hp.ragged(np.concatenate([hp.to_words([d for d, _ in rows], 5), hp.to_words([s for _, s in rows], 8)], axis=1))
    rows = rows + rows[:len(rec) - len(rows)]
    out = hp.run_whole_and_ragged("probe_base_digits", rec)
    check_base_output(out, rows, "base_digits")
    tops = hp.signed(out[:, [13, 18]])
    assert tops[:, 0].max() >= (1 << 21) - 1 and tops[:, 1].max() >= (1 << 15)      # the carry-absorbing tops are reached
    assert (np.abs(hp.signed(out[:, 8:13])) == 1 << 23).any()                       # a digit of -2^23: the last table index
    report("base_digits", len(rec), ", %d of them edge rows" % len(edges))


# ---- recodings --------------------------------------------------------------------------------
JOINT_HOST = os.path.join(ROOT, "tests", "cpp", "build", "joint_host_plain")


def joint_host_digits(rows):
    """geu_recode4 of the host build (tests/cpp/joint_host.cpp, built plain here: its sanitized build is
    tests/test_joint_table_host.py's): W digits per (x, W)."""
    os.makedirs(os.path.dirname(JOINT_HOST), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "narwhal_amd", "csrc"), "-o", JOINT_HOST,
                    os.path.join(ROOT, "tests", "cpp", "joint_host.cpp")], check=True)
    words = lambda x: " ".join(str((x >> (32 * i)) & 0xFFFFFFFF) for i in range(5))   # noqa: E731
    text = "\n".join("%d %s %s" % (W, words(x), words(x)) for x, W in rows) + "\n"
    r = subprocess.run([JOINT_HOST, "recode"], input=text, capture_output=True, text=True, timeout=120, check=True)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(rows)
    return [[int(v) for v in line.split()[:W]] for line, (x, W) in zip(lines, rows)]


def recode_rows(seed):
    """(x, W, W4): for every W in 33..37 and the joint counts 2W - 1 and 2W (W4 in 66..74 altogether; 65
    is below the ladder's range, so W = 33 pairs with 66 twice): 500 random x below the bound of the
    pair, every edge row that fits, and narrower values (the top windows are then zero)."""
    rng = random.Random(seed)
    rows = []
    for W in range(33, 38):
        for W4 in sorted({max(2 * W - 1, 66), 2 * W}):
            lim = min(4 * W - 1, 2 * W4 - 1)
            xs = [rng.getrandbits(lim) | (1 << (lim - 1)) for _ in range(250)]
            xs += [rng.getrandbits(lim) for _ in range(250)]
            xs += hm.recode_edges(lim)
            xs += [rng.getrandbits(b) for b in (1, 8, 64, 100, 120, 126, 127, 128, 129, 130, 131) for _ in range(4)]
            rows += [(x, W, W4) for x in xs]
    return rows


def check_recode_output(out, rows, host4=None):
    """Every string of one probe_half_recode output against the models; returns per radix the largest
    |digit| seen below the top and the largest top (for the ladders' safety check)."""
    o = hp.signed(out)
    seen = {"d16": 0, "top16": 0, "d256": 0, "d4": 0, "top4": 0}
    for i, (x, W, W4) in enumerate(rows):
        tag = "recode row %d (x = %d, W = %d, W4 = %d)" % (i, x, W, W4)
        want = hm.digits16(x, W)
        by_next = [int(v) for v in o[i, 6:6 + W - 1]] + [int(o[i, 5])]
        by_index = [int(v) for v in o[i, 42:42 + W - 1]] + [int(o[i, 5])]
        hm.check_digit_string(by_next, 4, x, 8, tag + " recode16/next16")
        assert by_next == want and by_index == want, tag + ": recode16 differs from the model"
        assert (out[i, 6 + W - 1:42] == hp.UNUSED).all() and (out[i, 42 + W - 1:78] == hp.UNUSED).all(), tag
        # the string's own words: digit w (w <= W - 2) as nibble w + 41 - W, nothing below the lowest digit
        packed = sum(int(v) << (32 * j) for j, v in enumerate(out[i, 0:5]))
        assert [((packed >> (4 * (w + 41 - W))) & 15) - 8 for w in range(W - 1)] == want[:-1], tag
        assert packed & ((1 << (4 * (41 - W))) - 1) == 0, tag
        nd = hm.ndig256(W)
        assert int(o[i, 102]) == nd, tag
        want = hm.digits256(x, nd)
        got = [int(v) for v in o[i, 83:83 + nd]]
        hm.check_digit_string(got[:-1] + [got[-1]], 8, x, 8, tag + " recode256/next256")
        assert got == want, tag + ": recode256 differs from the model"
        assert (out[i, 83 + nd:102] == hp.UNUSED).all(), tag
        want = hm.digits4(x, W4)
        got = [int(v) for v in o[i, 109:109 + W4 - 1]] + [int(o[i, 103])]
        hm.check_digit_string(got, 2, x, 2, tag + " geu_recode4/geu_digit4")
        assert got == want, tag + ": geu_recode4 differs from the model"
        assert (out[i, 109 + W4 - 1:182] == hp.UNUSED).all(), tag
        y = sum(int(v) << (32 * j) for j, v in enumerate(out[i, 104:109]))
        assert y == x + sum(2 << (2 * j) for j in range(W4 - 1)), tag + ": y words"
        if host4 is not None:
            assert got == host4[i], tag + ": geu_recode4 differs from the host build"
        seen["d16"] = max(seen["d16"], max(abs(v) for v in by_next[:-1]))
        seen["top16"] = max(seen["top16"], by_next[-1])
        seen["d256"] = max(seen["d256"], max(abs(v) for v in hm.digits256(x, nd)))
        seen["d4"] = max(seen["d4"], max(abs(v) for v in got[:-1]))
        seen["top4"] = max(seen["top4"], got[-1])
    return seen


def test_recodings():
    """recode16 + next16 + digit16_of, recode256 + next256, geu_recode4 + geu_digit4 at every window count."""
    t0 = time.time()
    rows = recode_rows(seed=16)
    out = hp.run_recode([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    seen = check_recode_output(out, rows, joint_host_digits([(x, W4) for x, _, W4 in rows]))
    assert seen == {"d16": 8, "top16": 8, "d256": 128, "d4": 2, "top4": 2}, seen   # every extreme digit is reached
    assert {W for _, W, _ in rows} == set(range(33, 38)) and {W4 for _, _, W4 in rows} == set(range(66, 75))
    report("recodings", len(rows), "; %.1f s" % (time.time() - t0))


# ---- window counts ----------------------------------------------------------------------------
def test_wave_windows():
    """Waves built lane by lane: all lanes equal, one wide lane at position 0, 31, 32 or 63 among narrow
    ones, for the bit lengths 0, 127, 130..147 and 148 (wave_windows' "38 if none"); and a ragged last
    wave, whose idle lanes sit on record 0."""
    lengths = [0, 127] + list(range(130, 149))
    waves = [[b] * 64 for b in lengths]
    for b in lengths:
        for pos in (0, 31, 32, 63):
            for narrow in (0, 127):
                w = [narrow] * 64
                w[pos] = b
                waves.append(w)
    last = [140] * 5                                            # ragged: record 0 (bit length 0) fills lanes 5..63
    flat = [b for w in waves for b in w] + last
    out = hp.run("probe_wave_windows", np.array(flat, dtype=np.uint32).reshape(-1, 1))
    for j, w in enumerate(waves + [last + [flat[0]]]):
        got = out[64 * j:64 * j + len(w)][:64]
        assert (got[:, 0] == hm.windows16(w)).all(), ("wave_windows", j, w, got[:, 0].tolist())
        assert (got[:, 1] == hm.windows4(w)).all(), ("wave_windows4", j, w, got[:, 1].tolist())
    assert set(out[:, 0].tolist()) == set(range(33, 39)) and set(out[:, 1].tolist()) == set(range(66, 75))
    report("window counts", len(flat), " in %d waves" % (len(waves) + 1))


# ---- ladders ----------------------------------------------------------------------------------
FEU_BOUND = np.tile(pp.FEU_TIGHT, 3)          # half_scalarmult: "X, Y, Z tight" (kernels.hip, verify_half)
FE_BOUND = np.tile(pp.TIGHT, 3)               # half_scalarmult_cached: ge_p1p1_to_p2's products are tight


@pytest.fixture(scope="module")
def ladder_setup():
    """The library with base24 built, a 16-key committee with known secret scalars, the record set and
    the scratch buffer; the committee is withdrawn afterwards."""
    import torch
    from narwhal_amd import _lib
    lib = _lib.load()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verify.json")))
    ok = next(c for c in gold["cases"] if c["name"] == "ref-verify_valid_signature")
    m, k, s = (bytes.fromhex(ok[f]) for f in ("msg", "pk", "sig"))
    assert lib.nwc_verify_strict(_lib.buf(m), _lib.buf(k), _lib.buf(s)) == 0
    rng = random.Random(1606)
    secrets = [rng.randrange(1, L) for _ in range(16)]
    keys = [ref.compress(ref.pt_mul(a, ref.BASEPOINT)) for a in secrets]
    recs = hm.ladder_records(seed=77, secrets=secrets)
    nonce = {}
    for r in recs:
        if r["r"] not in nonce:
            nonce[r["r"]] = ref.compress(ref.pt_mul(r["r"], ref.BASEPOINT))
    slots = (len(recs) + 255) // 256 * 256
    scratch = torch.zeros(slots * hp.SLOT_BYTES // 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.nwc_set_committee(_lib.buf(b"".join(keys)), len(keys)))
    try:
        base24, _ = pp.library_table("base24")
        tables, held = pp.library_table("committee_tables")
        assert base24 is not None and tables is not None and held == 16
        got_keys = pp.read_array(pp.library_table("committee_keys")[0])
        assert got_keys.astype("<u4").tobytes() == b"".join(keys)            # key i of the tables is key i given
        yield dict(recs=recs, keys=keys, nonce=nonce, scratch=scratch, slots=slots, base24=base24, tables=tables,
                   points=hm.t_points())
    finally:
        _lib.check(lib.nwc_set_committee(None, 0))


def ladder_words(setup, cached):
    rows = []
    for r in setup["recs"]:
        w = hp.to_words([r["c"]], 5)[0].tolist() + [r["c_neg"]] + hp.to_words([r["d"]], 5)[0].tolist()
        w += hp.to_words([r["s"]], 8)[0].tolist()
        w += [r["key"]] if cached else list(np.frombuffer(setup["keys"][r["key"]], dtype="<u4"))
        w += list(np.frombuffer(setup["nonce"][r["r"]], dtype="<u4"))
        rows.append(w)
    return np.array(rows, dtype=np.uint32)


def wave_W(recs, order, cached):
    """The model's window count of every record in launch order `order` (idle lanes of the last wave sit
    on the launch's record 0)."""
    W = np.empty(len(order), dtype=np.int64)
    for a in range(0, len(order), 64):
        lanes = [recs[i]["bits"] for i in order[a:a + 64]]
        if len(lanes) < 64:
            lanes.append(recs[order[0]]["bits"])
        W[a:a + 64] = (hm.windows16(lanes) | 1) if cached else hm.windows4(lanes)
    return W


def safe_to_launch(setup, orders, cached):
    """Before a ladder launch: the same records through probe_base_digits and probe_half_recode at the
    window counts of every launch order, and every index the ladder will form inside its table: base24
    (|digit| <= 2^23 in either half), the lane tables (9 entries; the joint one 13) and the key table (129)."""
    recs = setup["recs"]
    assert setup["base24"].elements == 2 * ((1 << 23) + 1)
    rec = np.concatenate([hp.to_words([r["d"] for r in recs], 5), hp.to_words([r["s"] for r in recs], 8)], axis=1)
    check_base_output(hp.run("probe_base_digits", rec), [(r["d"], r["s"]) for r in recs], "ladder records")
    triples = set()
    for order in orders:
        for i, W in zip(order, wave_W(recs, order, cached)):
            for x in (recs[i]["c"], recs[i]["d"]):
                triples.add((x, int(W), 2 * int(W)) if cached else (x, (int(W) + 1) // 2, int(W)))
    triples = sorted(triples)
    out = hp.run_recode([t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples])
    seen = check_recode_output(out, triples)
    assert seen["d16"] <= 8 and seen["top16"] <= 8 and seen["d256"] <= 128, seen           # 9 and 129 entries
    assert 5 * max(seen["d4"], seen["top4"]) + max(seen["d4"], seen["top4"]) <= 12, seen   # 13 joint entries
    assert all(r["bits"] <= hm.HALF_BITS and r["d"] & 1 and r["key"] < 16 for r in recs)
    return True


def run_ladder(setup, cached):
    recs = setup["recs"]
    name = "probe_half_ladder_cached" if cached else "probe_half_ladder_u"
    by_class = sorted(range(len(recs)), key=lambda i: (recs[i]["bits"], i))
    shuffled = list(range(len(recs)))
    random.Random(4242).shuffle(shuffled)
    orders = [by_class, shuffled]
    assert safe_to_launch(setup, orders, cached)
    words = ladder_words(setup, cached)
    par = hp.ladder_par(setup["scratch"], setup["slots"], setup["base24"], setup["tables"] if cached else None,
                        16 if cached else 0)
    bound = FE_BOUND if cached else FEU_BOUND
    results, seen_W = [], set()
    for order in orders:
        out = hp.run(name, words[order], par)
        want_W = wave_W(recs, order, cached)
        limbs = hp.signed(out[:, :30]) if cached else out[:, :30].astype(np.int64)
        res = [None] * len(recs)
        for pos, i in enumerate(order):
            r = recs[i]
            assert int(out[pos, 32]) == 1, "%s record %d: decode / contract flag %d" % (name, i, out[pos, 32])
            res[i] = hm.check_ladder_record(limbs[pos], out[pos, 30], out[pos, 31], setup["points"][r["t"]],
                                            int(want_W[pos]), bound, "%s record %d" % (name, i))
            seen_W.add(int(out[pos, 31]))
        results.append(res)
    for i, (a, b) in enumerate(zip(*results)):
        assert hm.same_projective(a, b), "%s record %d: the sorted and the shuffled launch disagree" % (name, i)
    idents = sum(1 for r in recs if r["t"] == 0)
    assert 3 * idents >= len(recs) - 2
    return len(recs), idents, sorted(seen_W)


def test_half_ladder_uncached(ladder_setup):
    """half_scalarmult (joint radix-4 table of A and R) over the grid of widths of (c, d)."""
    t0 = time.time()
    n, idents, Ws = run_ladder(ladder_setup, cached=False)
    assert Ws == list(range(66, 75)), Ws
    report("half_scalarmult", n, " x 2 launch orders, %d identities, W %s; %.1f s" % (idents, Ws, time.time() - t0))


def test_half_ladder_cached(ladder_setup):
    """half_scalarmult_cached (R's radix-16 table, the key's radix-256 table) over the same grid."""
    t0 = time.time()
    n, idents, Ws = run_ladder(ladder_setup, cached=True)
    assert Ws == [33, 35, 37], Ws
    report("half_scalarmult_cached", n, " x 2 launch orders, %d identities, W %s; %.1f s" % (idents, Ws, time.time() - t0))


# ---- coexistence ------------------------------------------------------------------------------
def test_probes_and_library_in_one_process():
    """Both probes and libnwc loaded together: a launch of each probe, then device.verify on the smoke
    fixture; the verdicts are what they are without the probes."""
    import torch
    from narwhal_amd import device
    pp.load()
    n = 4096
    msgs = device.derive32(b"smoke-msg", 0, n)
    pks, sigs = device.keygen_sign(device.derive32(b"smoke-seed", 0, n), msgs)
    sigs[::16, 40] ^= 1
    before = device.unpack_bits(device.verify(msgs, pks, sigs, strict=True), n)
    out = hp.run("probe_lat_reduce", hp.to_words([1, 2, L - 1], 8))
    assert hp.words_value(out[:2, 0:5]) == [1, 2] and hp.words_value(out[:2, 5:10]) == [1, 1]
    x = pp.run("probe_sc_lt_l", pp.to_words([L - 1, L], 8))
    assert x[:, 0].tolist() == [1, 0]
    after = device.unpack_bits(device.verify(msgs, pks, sigs, strict=True), n)
    torch.cuda.synchronize()
    assert (before == after).all() and int(after.sum()) == n - n // 16
