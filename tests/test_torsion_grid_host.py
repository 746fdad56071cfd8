"""The torsion grid (tests/golden/torsion_grid.json) and what tests/test_gpu_torsion_grid.py expects of
it, checked without a device.

  * every fixture vote's labels (a, b) re-derived with oracle/ed25519_ref.py, all 64 cells present, cell
    (0, 0) honest and the other 63 in dalek's randomized class;
  * the oracle's two evaluations of dalek's equation (term by term, and in Z/8) agree on every instance
    and seed the GPU tests use, and the Python restatement agrees on a sample;
  * conditions on the seeds: under each, the oracle alone accepts at least four and rejects at least four
    certificates (groups) of every randomized family, so both outcomes are pinned;
  * the mutation the repeated-key groups exist for -- a key's coefficient sum reduced mod l -- changes
    the verdict of at least one of them under every seed;
  * the Python mirror of straus_runs and the sub-batch cut against straus.h;
  * the grid probe (tests/hip/grid_probe.hip) carries the stamp of the tree's sources, exports exactly its
    entries, and a stale or missing library is told apart;
  * every probe checker accepts the right answer and rejects one wrong answer of every kind.
"""
import os
import random

import numpy as np
import pytest

from oracle import ed25519_ref as ref
from tests import grid_probe as gp
from tests import half_probe as hp
from tests import prim_probe as pp
from tests import torsion_grid as tg

L = ref.L


def rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ---- the fixture --------------------------------------------------------------------------------
def test_labels_rederived():
    g = tg.load_grid()
    msg = g.msg.tobytes()
    for b in range(8):
        A = ref.decompress(g.keys[b].tobytes())
        assert ref.torsion_dlog(ref.pt_mul(L, A)) == b, b
        for a in range(8):
            pk, sig = g.pk[a, b].tobytes(), g.sig[a, b].tobytes()
            assert ref.torsion_dlog(ref.residual(msg, pk, sig)) == a, (a, b)
            assert ref.vote_class(msg, pk, sig) == ("ok" if (a, b) == (0, 0) else "randomized"), (a, b)
    # eight distinct votes per key over the one message
    assert len({g.sig[a, b].tobytes() for a in range(8) for b in range(8)}) == 64
    assert len({g.keys[b].tobytes() for b in range(8)}) == 8


def test_oracle_classes_and_fillers(oracle):
    g = tg.load_grid()
    pks, sigs = g.pk.reshape(64, 32), g.sig.reshape(64, 64)
    cls = oracle.vote_class_many(np.tile(g.msg, (64, 1)), np.ascontiguousarray(pks), np.ascontiguousarray(sigs))
    assert cls.reshape(8, 8)[0, 0] == 0 and (np.delete(cls, 0) == 1).all()
    fp, fs = tg.fillers(oracle)
    assert len(fp) >= 8 and len(np.unique(fp, axis=0)) == len(fp)
    assert oracle.strict_many(np.tile(g.msg, (len(fp), 1)), fp, fs).all()
    assert fp[0].tobytes() == ref.public_key(g.filler_seeds[0].tobytes())
    assert ref.decompress(tg.undecodable_key()) is None


# ---- the instances ------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", tg.TAILS)
def test_resolve_instance_design(oracle, tail):
    inst = tg.instance(oracle, "resolve", tail)
    assert inst.nv % 64 == tail and inst.crafted[0] and inst.crafted[-1]
    single = inst.of_family("single")
    cells = {v[1:] for c in single for v in inst.votes[inst.offs[c]:inst.offs[c + 1]] if v[0] == "cell"}
    assert len(single) == 64 and cells == {(a, b) for a in range(8) for b in range(8)}
    per = lambda c: inst.votes[inst.offs[c]:inst.offs[c + 1]]   # noqa: E731
    assert sorted({sum(tg.crafted(v) for v in per(c)) for c in inst.of_family("multi")}) == [2, 3, 5, 8]
    onekey = inst.of_family("onekey")
    assert len(onekey) >= 8
    for c in onekey:
        assert len({v[2] for v in per(c) if v[0] == "cell"}) == 1 and sum(tg.crafted(v) for v in per(c)) >= 3
    assert {v[2] for c in onekey for v in per(c) if v[0] == "cell"} >= {1, 3, 5, 7}
    wide = inst.of_family("wide")
    assert len(wide) == 2 and all(inst.crafted[inst.offs[c]:inst.offs[c + 1]].sum() == 300 for c in wide)
    cls = oracle.vote_class_many(np.tile(inst.dig[0], (inst.nv, 1)), inst.pks, inst.sigs)
    assert ((cls == 1) == inst.crafted).all()
    for c in inst.of_family("err"):
        k = cls[inst.offs[c]:inst.offs[c + 1]]
        assert ((k == 2) | (k == -1)).sum() == 1 and (k == 1).any()
    # the committees: every key cached, or the fillers only
    assert len(tg.committee(oracle, True)) == len(tg.committee(oracle, False)) + 8


def test_group_instances_design(oracle):
    for name, groups, size in (("msm", tg.MSM_GROUPS, tg.MSM_GROUP), ("straus", tg.STRAUS_RUNS, tg.STRAUS_NQ)):
        inst = tg.instance(oracle, name)
        assert inst.m == groups and (np.diff(inst.offs) == size).all() and inst.crafted[0] and inst.crafted[-1]
        per = lambda c: inst.votes[inst.offs[c]:inst.offs[c + 1]]   # noqa: E731
        onekey = inst.of_family("onekey")
        assert len(onekey) >= 8
        for c in onekey:
            keys = {v[2] for v in per(c) if v[0] == "cell"}
            assert len(keys) == 1 and keys != {0} and sum(v[0] == "cell" for v in per(c)) >= 2
        assert len(inst.of_family("honest")) >= groups // 4 and len(inst.of_family("crafted")) == 4
        assert all(1 <= inst.crafted[inst.offs[c]:inst.offs[c + 1]].sum() <= 4 for c in inst.of_family("few"))


# ---- the oracle's two forms agree; conditions on the seeds ---------------------------------------
def _both(oracle, inst, seed, index=None, tag="call"):
    cert, bits = tg.expected(oracle, inst, seed, False, index, tag)
    cert8, bits8 = tg.expected(oracle, inst, seed, True, index, tag)
    assert (cert == cert8).all() and (bits == bits8).all(), (seed, np.nonzero(cert != cert8)[0][:8])
    return cert


def _both_outcomes(cert, which, what):
    acc = int(cert[which].sum())
    assert acc >= 4 and len(which) - acc >= 4, "%s: the oracle accepts %d of %d" % (what, acc, len(which))
    return acc


@pytest.mark.parametrize("tail", tg.TAILS)
def test_resolve_instance_seeds(oracle, tail):
    inst = tg.instance(oracle, "resolve", tail)
    single = [c for c in inst.of_family("single") if inst.crafted[inst.offs[c]:inst.offs[c + 1]].any()]
    assert len(single) == 63
    seeds = tg.SEEDS + ((tg.HOST_ENTRY_SEED,) if tail == 1 else ())
    for seed in seeds:
        cert = _both(oracle, inst, seed)
        a = _both_outcomes(cert, single, "seed %d singles" % seed)
        b = _both_outcomes(cert, inst.of_family("multi"), "seed %d multi" % seed)
        c = int(cert[inst.of_family("onekey")].sum())
        print("tail %d seed %d: accepted %d/63 singles, %d/128 multi, %d/16 one-key, %d/2 wide" % (
            tail, seed, a, b, c, int(cert[inst.of_family("wide")].sum())))
        assert not cert[inst.of_family("err")].any() and cert[inst.of_family("pad")].all()
        assert cert[[c for c in inst.of_family("single") if c not in single]].all()


def test_devices_seed_with_range_local_z(oracle):
    from narwhal_amd import shard
    inst = tg.instance(oracle, "resolve", 63)
    cuts = shard.cert_cuts(inst.offs, 2)
    assert 0 < cuts[1] < inst.nv
    idx = tg.local_index(inst.nv, cuts)
    assert idx[cuts[1]] == 0 and idx[cuts[1] - 1] == cuts[1] - 1 and idx[-1] == inst.nv - 1 - cuts[1]
    cert = _both(oracle, inst, tg.DEVICES_SEED, idx, "local2")
    fam = np.array(inst.families)
    rand = np.isin(fam, ("single", "multi", "onekey", "wide"))
    left = inst.offs[1:] <= cuts[1]
    for side in (left, ~left):
        _both_outcomes(cert, np.nonzero(rand & side)[0], "seed %d, one side of the cut" % tg.DEVICES_SEED)
    # the indices matter: the call's own indices give other verdicts behind the cut
    call = tg.expected(oracle, inst, tg.DEVICES_SEED)[0]
    assert (cert[left] == call[left]).all() and (cert[~left] != call[~left]).any()


def test_group_instances_seeds(oracle):
    for name in ("msm", "straus"):
        inst = tg.instance(oracle, name)
        rand = inst.of_family("onekey", "crafted", "few")
        for seed in tg.SEEDS:
            cert = _both(oracle, inst, seed)
            acc = _both_outcomes(cert, rand, "%s seed %d" % (name, seed))
            print("%s seed %d: the oracle accepts %d of %d crafted groups" % (name, seed, acc, len(rand)))
            assert cert[inst.of_family("honest")].all() and not cert[inst.of_family("err")].any()


def test_launches_call_seeds(oracle):
    dig, offs, pks, sigs, fam = tg.launches_call(oracle)
    fam = np.array(fam)
    nv = int(offs[-1])
    grid = np.nonzero(fam != "filler")[0]
    some = np.concatenate([grid, np.nonzero(fam == "filler")[0][::40]])
    for seed in tg.LAUNCH_SEEDS:
        zs = tg.zs_at(seed, np.arange(nv))
        sub_offs = np.concatenate([[0], np.cumsum(np.diff(offs)[some])])
        take = np.concatenate([np.arange(offs[c], offs[c + 1]) for c in some])
        a = tg.equation(oracle, dig[some], sub_offs, pks[take], sigs[take], zs[take], z8=False)
        b = tg.equation(oracle, dig[some], sub_offs, pks[take], sigs[take], zs[take], z8=True)
        assert (a == b).all() and a[len(grid):].all()
        rand = np.nonzero(np.isin(fam[grid], ("single", "multi", "wide", "straddle")))[0]
        _both_outcomes(a, rand, "launches seed %d" % seed)
        behind = np.nonzero(offs[:-1][grid] >= tg.MAX_LAUNCH)[0]
        _both_outcomes(a, np.intersect1d(rand, behind), "launches seed %d, second launch" % seed)
        print("launches seed %d: accepted %d of %d grid certificates, the straddling one: %s" % (
            seed, int(a[rand].sum()), len(rand), bool(a[np.nonzero(fam[grid] == "straddle")[0][0]])))


def test_python_restatement_on_a_sample(oracle):
    inst = tg.instance(oracle, "resolve", 0)
    seed = tg.SEEDS[0]
    cert = tg.expected(oracle, inst, seed)[0]
    zs = tg.zs_at(seed, np.arange(inst.nv))
    sample = inst.of_family("single")[3:60:20] + inst.of_family("multi")[::40] + inst.of_family("err")[:1]
    msg = inst.dig[0].tobytes()
    for c in sample:
        lo, hi = int(inst.offs[c]), int(inst.offs[c + 1])
        votes = [(inst.pks[v].tobytes(), inst.sigs[v].tobytes()) for v in range(lo, hi)]
        z = [int.from_bytes(zs[v].tobytes(), "little") for v in range(lo, hi)]
        assert z[0] == ref.batch_z(tg.seed_bytes(seed), lo)
        assert ref.verify_batch_z8(msg, votes, z) == bool(cert[c]), c


# ---- the mutation the repeated-key groups must see ----------------------------------------------
def test_reducing_a_key_sum_mod_l_is_visible(oracle):
    """msm.h sums a key's coefficients unreduced so that every vote keeps dalek's own.  Reduced mod l, the
    result moves by a multiple of l A_j: for every seed the GPU test uses, that changes the verdict of at
    least one repeated-key group of its instance.  Honest votes add nothing to the equation, so the
    Python evaluation runs on a group's crafted votes; that it then equals the oracle's verdict on the
    whole group is asserted too."""
    inst = tg.instance(oracle, "msm")
    msg = inst.dig[0].tobytes()
    for seed in tg.SEEDS:
        cert = tg.expected(oracle, inst, seed)[0]
        zs = tg.zs_at(seed, np.arange(inst.nv))
        seen = 0
        for c in inst.of_family("onekey"):
            vs = [v for v in range(int(inst.offs[c]), int(inst.offs[c + 1])) if inst.votes[v][0] == "cell"]
            votes = [(inst.pks[v].tobytes(), inst.sigs[v].tobytes()) for v in vs]
            z = [int.from_bytes(zs[v].tobytes(), "little") for v in vs]
            exact, mutated = tg.python_equation(msg, votes, z)
            assert exact == bool(cert[c]), (seed, c)
            seen += mutated != exact
        print("seed %d: reducing the key sums mod l changes %d of %d repeated-key groups" % (
            seed, seen, len(inst.of_family("onekey"))))
        assert seen >= 1, seed


def test_the_grid_tells_wrong_resolutions_apart(oracle):
    """The resolution on integers: a crafted vote's labels (a, b) are the fixture's, k is one SHA-512, and
    a certificate passes iff sum (z a + q b) = 0 mod 8 with q = floor(z k / l).  That model equals the
    oracle on every certificate without a deterministic failure; and each wrong variant of it -- a term
    dropped, q taken with 1 / l = 1 or from k's low bits alone, z of the neighbouring vote, z mod 4 --
    changes at least one certificate under every seed, so the GPU test would see the same mistake in
    k_vote_resolve."""
    import hashlib
    inst = tg.instance(oracle, "resolve", 0)
    msg = inst.dig[0].tobytes()
    cells = [(v, inst.votes[v][1], inst.votes[v][2]) for v in range(inst.nv) if inst.votes[v][0] == "cell"]
    ks = {v: int.from_bytes(hashlib.sha512(inst.sigs[v, :32].tobytes() + inst.pks[v].tobytes() + msg).digest(), "little") % L
          for v, _, _ in cells}
    cert_of = np.repeat(np.arange(inst.m), np.diff(inst.offs))
    plain = [c for c in range(inst.m) if inst.families[c] != "err"]

    def z_of(seed, v):
        return int.from_bytes(hashlib.sha512(tg.seed_bytes(seed) + v.to_bytes(8, "little")).digest()[:16], "little")

    variants = {
        "exact": lambda z, k, a, b, zn: z * a + (z * k // L) * b,
        "no z a": lambda z, k, a, b, zn: (z * k // L) * b,
        "no q b": lambda z, k, a, b, zn: z * a,
        "1 / l = 1": lambda z, k, a, b, zn: z * a + (z * k - z * k % L) * b,
        "q from the low bits of z k": lambda z, k, a, b, zn: z * a + 5 * ((z % 8) * (k % 8)) * b,
        "z of the next vote": lambda z, k, a, b, zn: zn * a + (zn * k // L) * b,
        "z mod 4": lambda z, k, a, b, zn: (z % 4) * a + (z * k // L) * b,
        "a and b swapped": lambda z, k, a, b, zn: z * b + (z * k // L) * a,
    }
    for seed in tg.SEEDS:
        ocert = tg.expected(oracle, inst, seed)[0]
        for name, f in variants.items():
            total = np.zeros(inst.m, dtype=np.int64)
            for v, a, b in cells:
                total[cert_of[v]] += f(z_of(seed, v), ks[v], a, b, z_of(seed, v + 1)) % 8
            verdict = total % 8 == 0
            if name == "exact":
                assert (verdict[plain] == ocert[plain]).all(), seed
            else:
                assert (verdict[plain] != ocert[plain]).any(), (seed, name)


# ---- the Straus cut -----------------------------------------------------------------------------
def test_straus_cut_mirror():
    max_per_lane, waves = tg.straus_constants()
    assert (max_per_lane, waves) == (16, 2)
    nv = tg.STRAUS_NQ * tg.STRAUS_RUNS
    # any device with at least one CU has 512 resident lanes or more: want = nv / nq <= lanes
    for lanes in (512, 256 * 512):
        assert tg.straus_runs(nv, lanes, tg.STRAUS_NQ, max_per_lane) == tg.STRAUS_RUNS
    assert tg.straus_cuts(nv, tg.STRAUS_RUNS) == list(range(0, nv + 1, tg.STRAUS_NQ))
    # the other branch of straus_runs: more runs wanted than lanes -> whole rounds, never above the maximum
    assert tg.straus_runs(100000, 512, 8, 16) == 24 * 512 and tg.straus_runs(16 * 512 + 1, 512, 16, 16) == 2 * 512
    assert tg.straus_runs(10, 512, 0, 16) == 10 and tg.straus_runs(1000, 512, 99, 16) == 63
    assert tg.straus_cuts(10, 3) == [0, 3, 6, 10]


# ---- probe entries and their checkers -----------------------------------------------------------
def test_grid_probe_build_and_stamp(tmp_path, monkeypatch):
    """The library build() left in the tree (built here if the tree has none) carries the stamp of the
    present sources and exports exactly its entries; a stale or missing one is told apart; the first two
    probes and the library do not depend on it."""
    import subprocess
    from narwhal_amd import build as nb
    out = gp.build_probe()
    assert gp.embedded_probe_id(out) == gp.probe_source_id() and gp.probe_up_to_date(out)
    syms = subprocess.run(["nm", "-D", "--defined-only", out], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(gp.ENTRIES) | {"probe_record_words", "probe_build_id"}, sorted(exported)
    assert set(gp.ENTRIES) == {"probe_torsion_dlog", "probe_mul_l", "probe_zq", "probe_zq_direct"}
    src = open(gp.SRC).read()
    for name in gp.ENTRIES:
        assert "(%s, k_gp_" % name in src and '{"%s",' % name in src, name
    assert src.count("hipLaunchKernelGGL(") == 1 and "k_verify" not in src.split("namespace {", 1)[1]
    for fn in ("torsion_dlog(", "ge_mul_l(", "straus_z(", "sc_mul128(", "resolve_q8("):
        assert fn in src.split("namespace {", 1)[1], fn
    names = {s.split("/")[-1] for s in gp.probe_sources()}
    assert {"resolve.h", "straus.h", "kernels.hip", "grid_probe.hip"} <= names
    assert gp.SRC not in nb.sources() and gp.SRC not in hp.probe_sources() and gp.SRC not in pp.probe_sources()
    # the kernel calls the helper the probe calls
    res = open(os.path.join(tg.ROOT, "narwhal_amd", "csrc", "resolve.h")).read()
    assert res.count("resolve_q8(") == 2 and "resolve_q8(z, kw, zk)" in res.split("void k_vote_resolve", 1)[1]
    # stale, missing, another probe's marker, a flag
    stale = tmp_path / "stale.so"
    stale.write_bytes(b"\x7fELF....NWC_GRID_PROBE_ID:0123456789abcdef0123\0....")
    assert gp.embedded_probe_id(str(stale)) == "0123456789abcdef0123" and not gp.probe_up_to_date(str(stale))
    assert not gp.probe_up_to_date(str(tmp_path / "missing.so"))
    assert hp.embedded_probe_id(str(stale)) is None and pp.embedded_probe_id(str(stale)) is None
    assert gp.embedded_probe_id(hp.OUT) is None
    before = gp.probe_source_id()
    monkeypatch.setattr(hp, "EXTRA_FLAGS", hp.EXTRA_FLAGS + ["-DX"])
    assert gp.probe_source_id() != before


def test_dlog_checker():
    rec, want = tg.dlog_rows()
    assert rec.shape[1] == gp.ENTRIES["probe_torsion_dlog"][0] and len(rec) > 256
    assert set(want.tolist()) == set(range(9)) and all((want == j).sum() >= 15 for j in range(8))
    # the rows state their points: X / Z and Y / Z of a torsion row are that torsion point's
    from tests.half_model import limb_value
    T = tg.torsion_points()
    for r, j in list(zip(rec, want))[:240]:
        x, y, z = (limb_value(r[10 * i:10 * i + 10]) for i in range(3))
        assert z and (x * pow(z, -1, ref.P) % ref.P, y * pow(z, -1, ref.P) % ref.P) == T[j]
    assert int(np.abs(rec.astype(np.int64)).max()) <= int(1.65 * (1 << 26))      # the loose bound
    tg.check_dlog(want.copy(), want)
    wrong = want.copy()
    wrong[5] = (wrong[5] + 1) % 8
    rejects(tg.check_dlog, wrong, want)
    wrong = want.copy()
    wrong[-1] = 0                     # a point outside E[8] taken for the identity
    rejects(tg.check_dlog, wrong, want)
    wrong = want.copy()
    wrong[0] = 8                      # the identity not found
    rejects(tg.check_dlog, wrong, want)


def test_mul_l_checker():
    rec, want, flag = tg.mul_l_rows()
    assert rec.shape[1] == gp.ENTRIES["probe_mul_l"][0]
    assert set(want[flag == 1].tolist()) == set(range(8)) and (flag == 0).sum() == 1
    # l (n B + T[j]) = [5 j] G8: the expectation, on a few rows, by the Python group law
    for i in (0, 13, 127, 263):
        Pt = ref.decompress(rec[i].astype("<u4").tobytes())
        assert ref.torsion_dlog(ref.pt_mul(L, Pt)) == want[i]
    right = np.stack([want, flag], axis=1)
    tg.check_mul_l(right, want, flag)
    garbage = right.copy()
    garbage[-1, 0] = 5                # the undecodable row's dlog is not read
    tg.check_mul_l(garbage, want, flag)
    wrong = right.copy()
    wrong[12, 0] = (wrong[12, 0] + 4) % 8
    rejects(tg.check_mul_l, wrong, want, flag)
    wrong = right.copy()
    wrong[3, 0] = 8
    rejects(tg.check_mul_l, wrong, want, flag)
    wrong = right.copy()
    wrong[-1, 1] = 1                  # the undecodable key reported as decoded
    rejects(tg.check_mul_l, wrong, want, flag)


def _zq_words(z, k):
    zk, q8 = z * k % L, (z * k // L) % 8
    return [(z >> (32 * i)) & 0xFFFFFFFF for i in range(4)] + [(zk >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [q8]


def test_zq_checkers():
    import hashlib
    rec, cases = tg.zq_rows()
    assert rec.shape[1] == gp.ENTRIES["probe_zq"][0] and len(rec) > 256
    assert any(v >= 1 << 32 for _, v, _ in cases) and {0, L - 1} <= {k for _, _, k in cases}
    right = np.array([_zq_words(int.from_bytes(hashlib.sha512(s + v.to_bytes(8, "little")).digest()[:16], "little"), k)
                      for s, v, k in cases], dtype=np.uint32)
    tg.check_zq(right, cases)
    # the z of the knob's seed is the one the verdict tests derive
    s, v, k = tg.seed_bytes(11), 5, 1
    assert _zq_words(ref.batch_z(s, v), k)[:4] == list(np.frombuffer(tg.zs_at(11, [v]).tobytes(), "<u4"))
    for col, what in ((0, "z"), (3, "z high word"), (4, "z k mod l"), (11, "z k mod l high word"), (12, "q8")):
        wrong = right.copy()
        wrong[40, col] ^= 1
        rejects(tg.check_zq, wrong, cases)
    # v's high word dropped (v >= 2^32 hashed as v mod 2^32)
    i = next(i for i, (_, v, _) in enumerate(cases) if v >= 1 << 32)
    s, v, k = cases[i]
    wrong = right.copy()
    wrong[i] = _zq_words(ref.batch_z(s, v & 0xFFFFFFFF), k)
    rejects(tg.check_zq, wrong, cases)
    drec, dcases = tg.zq_direct_rows()
    assert drec.shape[1] == gp.ENTRIES["probe_zq_direct"][0]
    assert {0, (1 << 128) - 1} <= {z for z, _ in dcases} and {0, L - 1} <= {k for _, k in dcases}
    dright = np.array([_zq_words(z, k) for z, k in dcases], dtype=np.uint32)
    tg.check_zq_direct(dright, dcases)
    j = next(i for i, (z, k) in enumerate(dcases) if z == (1 << 128) - 1 and k == L - 1)
    wrong = dright.copy()
    wrong[j, 12] = (wrong[j, 12] + 5) % 8      # q taken with 1 / l = 1 instead of 5, say
    rejects(tg.check_zq_direct, wrong, dcases)
    wrong = dright.copy()
    wrong[j, 4:12] = [(((1 << 128) - 1) * (L - 1) % (1 << 256) >> (32 * i)) & 0xFFFFFFFF for i in range(8)]   # unreduced
    rejects(tg.check_zq_direct, wrong, dcases)
    # q8 is a function of the low bits only when z k mod l is right: every value 0..7 occurs
    assert {int(r[12]) for r in dright} == set(range(8))
    rng = random.Random(1)
    for _ in range(200):      # the kernel's three-line formula, on integers
        z, k = rng.getrandbits(128), rng.randrange(L)
        assert (5 * (((z & 7) * (k & 7) + 8 - (z * k % L & 7)) & 7)) & 7 == (z * k // L) % 8
