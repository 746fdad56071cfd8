"""The models and checks of tests/test_gpu_half.py, tested without a device.

  * the half-size probe (tests/hip/half_probe.hip) cross-compiles from a clean tree with the library's
    flags, exports exactly its entries, is no source of libnwc.so, and a missing or stale library is
    told apart (tests/half_probe.load() then fails; nothing skips);
  * the integer models of tests/half_model.py against each other and against the host build of
    lattice.h, and the class population of the constructed challenges;
  * every checker accepts the model's right answer and rejects one wrong answer of every kind it
    claims to catch: a digit out of range, a lost carry, a wrong top digit, d even, a wrong sign, bits
    off by one, a point off by B, a stale ident.
"""
import random
import subprocess

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import half_model as hm
from tests import half_probe as hp
from tests import prim_probe as pp

P, L, N = hm.P, hm.L, hm.N


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ---- probe build ------------------------------------------------------------------------------
def test_half_probe_builds_and_exports_its_entries(tmp_path):
    from narwhal_amd import build as nb
    out = hp.build_probe(out=str(tmp_path / "libnwc_half_probe.so"), force=True)
    assert hp.embedded_probe_id(out) == hp.probe_source_id()
    assert hp.probe_up_to_date(out)
    syms = subprocess.run(["nm", "-D", "--defined-only", out], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    # the entries and nothing else: no function of kernels.hip or of the csrc headers leaves the library
    assert exported == set(hp.ENTRIES) | {"probe_record_words", "probe_build_id", "probe_ladder_par_words",
                                          "probe_ladder_slot_bytes"}, sorted(exported)
    src = open(hp.SRC).read()
    for name in hp.ENTRIES:
        assert "(%s, k_hp_" % name in src and '{"%s",' % name in src, name
    # every kernel the probe launches is its own: the launches name k_hp_* kernels only
    assert src.count("hipLaunchKernelGGL(") == 2 and "k_verify" not in src.split("namespace {", 1)[1]
    # the library's build id does not depend on the probe, the probe's depends on the library's kernels and flags
    assert all("tests" not in s.split("/") for s in nb.sources()) and hp.SRC not in nb.sources()
    names = {s.split("/")[-1] for s in hp.probe_sources()}
    assert {"half_probe.hip", "kernels.hip", "lattice.h", "ge_u25519.h", "sha512.h"} <= names
    assert set(hp.EXTRA_FLAGS) <= set(hp.probe_flags()) and set(nb.FLAGS) <= set(hp.probe_flags())


def test_a_stale_half_probe_is_told_apart(tmp_path, monkeypatch):
    stale = tmp_path / "stale.so"
    stale.write_bytes(b"\x7fELF....NWC_HALF_PROBE_ID:0123456789abcdef0123\0....")
    assert hp.embedded_probe_id(str(stale)) == "0123456789abcdef0123"
    assert not hp.probe_up_to_date(str(stale))
    assert not hp.probe_up_to_date(str(tmp_path / "missing.so"))
    # the first probe's marker is another one: neither library passes for the other
    assert pp.embedded_probe_id(str(stale)) is None
    # a flag is part of the stamp
    before = hp.probe_source_id()
    monkeypatch.setattr(hp, "EXTRA_FLAGS", hp.EXTRA_FLAGS + ["-DX"])
    assert hp.probe_source_id() != before


# ---- lat::reduce ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lat():
    return hm.host_lattice()


def test_euclid_rows_and_model_against_the_host_build(host_lat):
    ks = hm.ordinary_k()
    ks = ks[:3000] + ks[20000:21000] + ks[23000:]
    even = 0
    for k in ks:
        (r0, t0), (r1, t1) = hm.euclid(k)
        assert r1 < 1 << 127 and (r0 >= 1 << 127 or k < 1 << 127)
        assert (t0 * k - r0) % N == 0 and (t1 * k - r1) % N == 0
        assert abs(r0 * t1 - r1 * t0) == N
        c_abs, d, neg, ok = hm.host_reduce(host_lat, k)
        hm.check_half_scalars(k, c_abs, d, neg, ok, max(c_abs.bit_length(), d.bit_length()), "host")
        if ok:
            hm.check_against_model(k, c_abs, d, neg, "host")
        mc, md, mok, m = hm.model_reduce(k)
        # the host build may also give up on its iteration budget (k = 2^127: one quotient of 2^128)
        assert mok or not ok, k
        if ok:
            assert (mc, md) == (-c_abs if neg else c_abs, d), k
        if m is not None:
            even += 1
            if ok:   # with ok clear c may be wider than the five words the result holds
                assert hm.even_branch_m(k, c_abs, d, neg) == m
    assert even > len(ks) // 4


def test_constructed_k_reach_every_width(host_lat):
    """The class-population condition of tests/test_gpu_half.py's constructed set, by the host build (both
    of its reductions, which must agree) and by the model."""
    ks = hm.constructed_k(seed=2146)
    assert len(ks) == 1280 and all(0 < k < L for k in ks)
    widths, oks = [], []
    for k in ks:
        (r0, t0), (r1, t1) = hm.euclid(k)
        assert t1 % 2 == 0 and 96 <= abs(t1).bit_length() <= 127
        h = hm.host_reduce(host_lat, k)
        assert h == hm.host_reduce(host_lat, k, "lat_reduce_single"), k
        hm.check_half_scalars(k, h[0], h[1], h[2], h[3], max(h[0].bit_length(), h[1].bit_length()), "host")
        mc, md, mok, m = hm.model_reduce(k)
        assert mok == bool(h[3]), k
        assert (mc, md) == (-h[0] if h[2] else h[0], h[1]) or not mok, k
        widths.append(max(h[0].bit_length(), h[1].bit_length()))
        oks.append(h[3])
    hm.check_population(widths, oks)
    per, failed = hm.class_counts(widths, oks)
    print("constructed k: ok per width %s, %d with ok clear" % (sorted(per.items()), failed))
    # and the condition itself can fail
    rejects(hm.check_population, [w for w in widths if w != 140], [o for w, o in zip(widths, oks) if w != 140])
    rejects(hm.check_population, widths, [1] * len(oks))


def test_half_scalar_checker_rejects_each_kind():
    rng = random.Random(3)
    k = rng.randrange(L)
    c, d, ok, _ = hm.model_reduce(k)
    assert ok
    c_abs, neg, bits = abs(c), int(c < 0), max(abs(c).bit_length(), d.bit_length())
    hm.check_half_scalars(k, c_abs, d, neg, 1, bits)
    hm.check_against_model(k, c_abs, d, neg)
    rejects(hm.check_half_scalars, k, c_abs, d, 1 - neg, 1, bits)                   # a wrong sign
    rejects(hm.check_half_scalars, k, c_abs, d, neg, 1, bits + 1)                   # bits off by one
    rejects(hm.check_half_scalars, k, c_abs, d, neg, 1, bits - 1)
    rejects(hm.check_half_scalars, k, 2 * c_abs, 2 * d, neg, 1, bits + 1)           # d even (the relation still holds)
    rejects(hm.check_half_scalars, k, 0, 0, 0, 1, 0)                                # c = d = 0 with ok set
    rejects(hm.check_half_scalars, k, c_abs + 1, d, neg, 1, max((c_abs + 1).bit_length(), d.bit_length()))
    rejects(hm.check_half_scalars, 0, 0, 1, 1, 1, 1)                                # c = 0 with the sign set
    wide_c, wide_d = abs(c) * ((1 << 20) + 1), d * ((1 << 20) + 1)
    rejects(hm.check_half_scalars, k, wide_c, wide_d, neg, 1, max(wide_c.bit_length(), wide_d.bit_length()))   # out of range
    hm.check_half_scalars(k, wide_c, wide_d, neg, 0, max(wide_c.bit_length(), wide_d.bit_length()))             # fine with ok clear
    # another sound pair than Euclid's row is not the model's
    odd = next(kk for kk in (rng.randrange(L) for _ in range(100)) if hm.euclid(kk)[1][1] & 1)
    c, d, ok, m = hm.model_reduce(odd)
    assert m is None
    rejects(hm.check_against_model, odd, (3 * abs(c)), 3 * d, int(c < 0))


# ---- digit strings ----------------------------------------------------------------------------
def test_digit_models_and_their_checker():
    rng = random.Random(4)
    for W in range(33, 38):
        for x in hm.recode_edges(4 * W - 1) + [rng.getrandbits(4 * W - 1) for _ in range(200)]:
            hm.check_digit_string(hm.digits16(x, W), 4, x, 8)
            hm.check_digit_string(hm.digits256(x, hm.ndig256(W)), 8, x, 8)
    for W in range(66, 75):
        for x in hm.recode_edges(2 * W - 1) + [rng.getrandbits(2 * W - 1) for _ in range(200)]:
            hm.check_digit_string(hm.digits4(x, W), 2, x, 2)
    # radix 4 against radix 16: two joint windows are one radix-16 window up to the carry between them
    x = rng.getrandbits(139)
    d4, d16 = hm.digits4(x, 70), hm.digits16(x, 35)
    assert sum(v << (2 * i) for i, v in enumerate(d4)) == sum(v << (4 * i) for i, v in enumerate(d16)) == x
    assert hm.ndig256(33) == 17 and hm.ndig256(34) == hm.ndig256(35) == 18 and hm.ndig256(36) == hm.ndig256(37) == 19
    good = hm.digits16(x, 35)
    hm.check_digit_string(good, 4, x, 8)
    bad = list(good); bad[3] += 16; bad[4] -= 1                                     # a digit out of range, the sum still right
    assert sum(v << (4 * i) for i, v in enumerate(bad)) == x
    rejects(hm.check_digit_string, bad, 4, x, 8)
    y = (1 << 139) - 1                                                              # every carry taken, the top digit 8
    good = hm.digits16(y, 35)
    assert good[-1] == 8 and good[0] == -1
    lost = list(good); lost[-1] -= 1                                                # the carry into the top lost
    rejects(hm.check_digit_string, lost, 4, y, 8)
    lost = list(good); lost[7] -= 1                                                 # a carry lost inside the string
    rejects(hm.check_digit_string, lost, 4, y, 8)
    top = list(good); top[-1] = 9; top[-2] -= 16                                    # a wrong top digit, the sum still right
    assert sum(v << (4 * i) for i, v in enumerate(top)) == y
    rejects(hm.check_digit_string, top, 4, y, 8)
    assert hm.windows16([0]) == 33 and hm.windows16([131, 5]) == 33 and hm.windows16([132]) == 34
    assert hm.windows16([147]) == 37 and hm.windows16([148]) == 38
    assert hm.windows4([131]) == 66 and hm.windows4([132]) == 67 and hm.windows4([146]) == 74 and hm.windows4([148]) == 74


def test_base_digit_model_and_its_checker():
    rows = hm.base_digit_edges(seed=24) + hm.random_base_rows(seed=25, n=300)
    assert all(d & 1 and 0 < d < 1 << 146 and 0 <= s < L for d, s in rows)
    assert {d.bit_length() for d, _ in rows} >= set(range(128, 147)) | {1}
    es = {d * s % L for d, s in rows}
    assert {0, 1, L - 1, (1 << 141) - 1, 1 << 141} <= es and any(s == L - 1 for _, s in rows)
    for d, s in rows:
        e = d * s % L
        el, eh = hm.base_digit_model(e)
        hm.check_base_digits(e, el, eh, d, s)
    d, s = rows[40]
    e = d * s % L
    el, eh = hm.base_digit_model(e)
    rejects(hm.check_base_digits, (e + 1) % L, el, eh, d, s)                        # eb itself wrong
    bad = list(el); bad[1] += 1 << 24; bad[2] -= 1                                  # a digit out of range, the sum still right
    rejects(hm.check_base_digits, e, bad, eh, d, s)
    bad = list(el); bad[2] += 1                                                     # a carry too many
    rejects(hm.check_base_digits, e, bad, eh, d, s)
    bad_l, bad_h = list(el), list(eh); bad_l[5] -= 1 << 21; bad_h[0] += 1           # 2^141 moved across the split
    assert sum(v << (24 * i) for i, v in enumerate(bad_l)) + (sum(v << (24 * i) for i, v in enumerate(bad_h)) << 141) == e
    rejects(hm.check_base_digits, e, bad_l, bad_h, d, s)
    # the top digit of the low half reaches 2^21 (the carry), never the table's end
    el, _ = hm.base_digit_model((1 << 141) - 1)
    assert el == [-1, 0, 0, 0, 0, 1 << 21]


# ---- ladders ----------------------------------------------------------------------------------
def test_ladder_records_and_their_checker():
    rng = random.Random(6)
    secrets = [rng.randrange(1, L) for _ in range(16)]
    recs = hm.ladder_records(seed=77, secrets=secrets)
    assert 1800 <= len(recs) <= 2200
    cls = lambda v: max(v.bit_length(), 127)   # noqa: E731
    assert {(cls(r["c"]), cls(r["d"]), r["c_neg"]) for r in recs} >= {(a, b, n) for a in hm.WIDTH_CLASSES
                                                                     for b in hm.WIDTH_CLASSES for n in (0, 1)}
    assert 3 * sum(1 for r in recs if r["t"] == 0) >= len(recs) - 2
    for r in recs[::37]:
        c = -r["c"] if r["c_neg"] else r["c"]
        assert r["d"] & 1 and r["bits"] <= 146 and 0 <= r["s"] < L
        assert (r["d"] * r["s"] - c * secrets[r["key"]] - r["d"] * r["r"] - r["t"]) % L == 0
    pts = hm.t_points()
    assert pts[0] == (0, 1) and pts[1] == ref.BASEPOINT and pts[L - 1] == ((-ref.BASEPOINT[0]) % P, ref.BASEPOINT[1])
    bound = np.tile(pp.FEU_TIGHT, 3)

    def limbs(pt, z):
        return pp.limbs_of(pt[0] * z % P) + pp.limbs_of(pt[1] * z % P) + pp.limbs_of(z)

    z = rng.randrange(1, P)
    seven = limbs(pts[7], z)
    got = hm.check_ladder_record(seven, 0, 70, pts[7], 70, bound)
    assert hm.same_projective(got, hm.check_ladder_record(limbs(pts[7], 5), 0, 70, pts[7], 70, bound))
    assert not hm.same_projective(got, hm.check_ladder_record(limbs(pts[2], 5), 0, 70, pts[2], 70, bound))
    eight = limbs(ref.pt_add(pts[7], ref.BASEPOINT), z)
    rejects(hm.check_ladder_record, eight, 0, 70, pts[7], 70, bound)                # a point off by B
    rejects(hm.check_ladder_record, seven, 1, 70, pts[7], 70, bound)                # a stale ident
    rejects(hm.check_ladder_record, limbs(pts[0], z), 0, 70, pts[0], 70, bound)     # the identity not flagged
    hm.check_ladder_record(limbs(pts[0], z), 1, 70, pts[0], 70, bound)
    rejects(hm.check_ladder_record, seven, 0, 71, pts[7], 70, bound)                # another window count
    rejects(hm.check_ladder_record, [0] * 30, 1, 70, pts[0], 70, bound)             # Z = 0
    over = list(seven); over[3] += 1 << 27                                          # a limb past tight
    rejects(hm.check_ladder_record, over, 0, 70, pts[7], 70, bound)
