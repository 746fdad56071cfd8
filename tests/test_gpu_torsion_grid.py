"""dalek's batch equation on the GPU, held exactly to the oracle on a grid that spans E[8] x E[8]
(crypto/src/lib.rs:206-219 -> ed25519-dalek 1.0.1 verify_batch; narwhal_amd/csrc/resolve.h, msm.h,
straus.h).

Only on the dalek-semantics entries can a crafted vote be accepted, so a wrong answer there is a forged
certificate passing.  tests/golden/torsion_grid.json holds one vote for every pair (residual
e = [a] G8, key with l A = [b] G8); tests/torsion_grid.py builds certificates, Pippenger groups and
Straus sub-batches from them and says, from the oracle's term-by-term evaluation for the z_i of a fixed
`dalek_seed`, what each must answer.  Nothing here is statistical and no expectation comes from the
device:

  * the primitives alone, through the grid probe (tests/hip/grid_probe.hip): torsion_dlog on every
    torsion point in several projective scalings and limb forms and on points outside E[8]; ge_mul_l on
    n B + T[j]; straus_z, sc_mul128 and resolve_q8 against hashlib and integers (v >= 2^32, k = 0 and
    l - 1, z = 0 and 2^128 - 1);
  * the per-certificate resolution with every key's comb, and with the grid's keys on the ladder in the
    same waves as cached keys: five seeds, nv % 64 in {0, 1, 63}; all 64 cells alone, certificates of
    2..8 and of 300 crafted votes, one key's votes together, torsion beside a deterministic failure;
  * the host entry; 64 Pippenger groups of 64 votes, with repeated torsion-bearing keys, counted by
    nwc_msm_stats, also right after the skip policy was armed and turned off; 128 Straus sub-batches of 8;
  * in child processes: a call cut into two launches (z indexed by the call's vote index, a certificate
    astride the cut) and two device contexts (z indexed within a device's range).

tests/test_torsion_grid_host.py checks the fixture, the expectations and the seeds without a device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import grid_probe as gp
from tests import torsion_grid as tg
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

HELPER = os.path.join(ROOT, "tests", "torsion_grid_helper.py")


def _bits(raw, n):
    return np.unpackbits(np.frombuffer(raw, np.uint8), bitorder="little")[:n].astype(bool)


# ---- the primitives -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    return gp.load()        # a missing or stale probe library is an error, not a skip


def test_torsion_dlog(probe):
    rec, want = tg.dlog_rows()
    out = gp.run_whole_and_ragged("probe_torsion_dlog", gp.ragged(rec))
    tg.check_dlog(out[:len(rec), 0], want)


def test_mul_l(probe):
    rec, want, flag = tg.mul_l_rows()
    out = gp.run_whole_and_ragged("probe_mul_l", gp.ragged(rec))
    tg.check_mul_l(out[:len(rec)], want, flag)


def test_z_and_q8(probe):
    rec, cases = tg.zq_rows()
    tg.check_zq(gp.run_whole_and_ragged("probe_zq", gp.ragged(rec))[:len(rec)], cases)
    rec, cases = tg.zq_direct_rows()
    tg.check_zq_direct(gp.run_whole_and_ragged("probe_zq_direct", gp.ragged(rec))[:len(rec)], cases)


# ---- the device entry ---------------------------------------------------------------------------
def _dev(entry, inst):
    """Leaf bits, certificate verdicts and bad votes of one call of a device entry."""
    import torch
    from narwhal_amd import device
    mi = np.repeat(np.arange(inst.m, dtype=np.int32), np.diff(inst.offs))
    t = lambda a, dt=torch.uint8: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()  # noqa: E731
    do = t(inst.offs.astype(np.int32), torch.int32)
    leaf = entry(t(inst.dig), do, t(mi, torch.int32), t(inst.pks), t(inst.sigs))
    cert, bad = device.cert_reduce(leaf, do, inst.nv)
    torch.cuda.synchronize()
    return device.unpack_bits(leaf, inst.nv), device.unpack_bits(cert, inst.m), device.unpack_bits(bad, inst.nv)


def _names(inst, cs):
    return [(int(c), inst.families[c], inst.votes[inst.offs[c]:inst.offs[c + 1]][:6]) for c in cs[:6]]


@pytest.mark.parametrize("tail", tg.TAILS)
@pytest.mark.parametrize("keys", ["comb", "ladder"])
def test_every_certificate_of_the_grid(oracle, keys, tail):
    """comb: the committee cache holds the fillers' and the grid's keys, so k_vote_resolve takes R' from
    the comb.  ladder: it holds the fillers' only; the grid's votes are uncached and the waves of the
    resolution hold both kinds (deterministic failures of cached keys beside them).  Every certificate's
    verdict and every vote's leaf bit equal dalek's equation for the same z_i."""
    from narwhal_amd import _lib, device
    lib = _lib.load()
    inst = tg.instance(oracle, "resolve", tail)
    cm = tg.committee(oracle, keys == "comb")
    try:
        _lib.check(lib.nwc_set_committee(_lib.buf(cm), len(cm)))
        for seed in tg.SEEDS:
            _lib.diag_set("dalek_seed", seed)
            leaf, cert, bad = _dev(device.verify_batch_msm, inst)
            ocert, obits = tg.expected(oracle, inst, seed)
            diff = np.nonzero(cert != ocert)[0]
            assert len(diff) == 0, (seed, _names(inst, diff))
            assert (leaf == obits).all(), (seed, np.nonzero(leaf != obits)[0][:10])
            assert (bad == ~obits).all()
    finally:
        _lib.diag_set("dalek_seed", 0)
        _lib.check(lib.nwc_set_committee(None, 0))


def test_host_entry(oracle):
    """nwc_verify_batch_msm_many (host buffers, one device range: vote indices are the call's)."""
    from narwhal_amd import _lib
    lib = _lib.load()
    inst = tg.instance(oracle, "resolve", 1)
    cm = tg.committee(oracle, True)
    cert = ctypes.create_string_buffer((inst.m + 7) // 8)
    badb = ctypes.create_string_buffer((inst.nv + 7) // 8)
    try:
        _lib.check(lib.nwc_set_committee(_lib.buf(cm), len(cm)))
        _lib.diag_set("dalek_seed", tg.HOST_ENTRY_SEED)
        _lib.check(lib.nwc_verify_batch_msm_many(_lib.buf(inst.dig), _lib.buf(inst.offs.astype(np.uint32)),
                                                 _lib.buf(inst.pks), _lib.buf(inst.sigs), inst.m, cert, badb))
    finally:
        _lib.diag_set("dalek_seed", 0)
        _lib.check(lib.nwc_set_committee(None, 0))
    ocert, obits = tg.expected(oracle, inst, tg.HOST_ENTRY_SEED)
    diff = np.nonzero(_bits(cert.raw, inst.m) != ocert)[0]
    assert len(diff) == 0, _names(inst, diff)
    assert (_bits(badb.raw, inst.nv) == ~obits).all()


def test_pippenger_groups(oracle):
    """No committee and fewer votes than launch keys need: k_verify_msm over 64 groups of 64 votes, z
    indexed by the call's vote index.  A group's votes pass iff dalek's equation holds over the group
    (a key that signs several of its votes keeps every vote's own coefficient: the sum is not reduced
    mod l), else each falls to its exact leaf; and the groups the equation passed and failed are counted,
    so a wrongly rejected honest group cannot hide behind the leaves."""
    from narwhal_amd import _lib, device
    inst = tg.instance(oracle, "msm")
    assert inst.nv == tg.MSM_GROUP * tg.MSM_GROUPS
    try:
        _lib.diag_set("msm_adapt", 0)
        _lib.diag_set("msm_group", tg.MSM_GROUP)
        for seed in tg.SEEDS:
            _lib.diag_set("dalek_seed", seed)
            p0, f0, o0 = device.msm_stats()[:3]
            leaf, _, _ = _dev(device.verify_batch_msm, inst)
            p1, f1, o1 = device.msm_stats()[:3]
            ogroup, obits = tg.expected(oracle, inst, seed)
            diff = np.nonzero(leaf != obits)[0]
            assert len(diff) == 0, (seed, _names(inst, sorted(set(diff // tg.MSM_GROUP))))
            assert (p1 - p0, f1 - f0, o1 - o0) == (int(ogroup.sum()), int((~ogroup).sum()), 0), (seed, p1 - p0, f1 - f0)
    finally:
        _lib.diag_set("dalek_seed", 0)
        _lib.diag_set("msm_group", 0)
        _lib.diag_set("msm_adapt", 1)


def test_policy_off_holds_for_the_next_launch(oracle):
    """msm_adapt = 0 means the equation on every group.  The skip policy's mode is device state: a
    launch with the policy on whose groups mostly fail (this instance: 48 of 64 hold crafted or bad
    votes) arms it, and a launch made after the policy is turned off must not obey it -- skipping hands
    every group to the leaves, which reject the crafted groups the equation accepts.  (This is the input
    on which test_pippenger_groups first differed from the oracle, run after tests that had armed the
    mode; the launch now takes the knob's value with it.)"""
    from narwhal_amd import _lib, device
    inst = tg.instance(oracle, "msm")
    seed = tg.SEEDS[0]
    ogroup, obits = tg.expected(oracle, inst, seed)
    assert ogroup[inst.of_family("onekey", "crafted", "few")].any()
    try:
        _lib.diag_set("msm_group", tg.MSM_GROUP)
        _lib.diag_set("msm_adapt", 1)
        for _ in range(9):      # until a launch measures (at most 7 skip first) and fails most of its groups
            f0 = device.msm_stats()[1]
            _dev(device.verify_batch_msm, inst)
            if device.msm_stats()[1] - f0 > tg.MSM_GROUPS // 2:
                break
        else:
            raise AssertionError("no launch ran the equation")
        _lib.diag_set("msm_adapt", 0)
        _lib.diag_set("dalek_seed", seed)
        s0 = device.msm_stats()
        leaf, _, _ = _dev(device.verify_batch_msm, inst)
        s1 = device.msm_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[3] - s0[3]) == (int(ogroup.sum()), int((~ogroup).sum()), 0), (s0, s1)
        assert (leaf == obits).all(), np.nonzero(leaf != obits)[0][:10]
    finally:
        _lib.diag_set("dalek_seed", 0)
        _lib.diag_set("msm_group", 0)
        _lib.diag_set("msm_adapt", 1)


def test_straus_sub_batches(oracle):
    """k_verify_straus with a target of 8 votes: 128 sub-batches of exactly 8 consecutive votes
    (tests/test_torsion_grid_host.py pins the cut), each decided by dalek's equation over its votes."""
    from narwhal_amd import _lib, device
    inst = tg.instance(oracle, "straus")
    assert inst.nv == tg.STRAUS_NQ * tg.STRAUS_RUNS
    try:
        _lib.diag_set("straus_nq", tg.STRAUS_NQ)
        for seed in tg.SEEDS:
            _lib.diag_set("dalek_seed", seed)
            leaf, _, _ = _dev(device.verify_batch_straus, inst)
            _, obits = tg.expected(oracle, inst, seed)
            diff = np.nonzero(leaf != obits)[0]
            assert len(diff) == 0, (seed, _names(inst, sorted(set(diff // tg.STRAUS_NQ))))
    finally:
        _lib.diag_set("dalek_seed", 0)
        _lib.diag_set("straus_nq", 12)


# ---- child processes ----------------------------------------------------------------------------
def _child(tmp_path, mode, env, seeds, **arrays):
    np.savez(tmp_path / "in.npz", seeds=np.array(seeds, np.int64), **arrays)
    subprocess.run([sys.executable, HELPER, mode, str(tmp_path / "in.npz"), str(tmp_path / "out.npz"), ROOT],
                   env=dict(os.environ, **env), check=True, timeout=300)
    return np.load(tmp_path / "out.npz")


def test_two_launches(oracle, tmp_path):
    """NWC_VERIFY_MAX_LAUNCH = 65,536 and a call of ~69,000 votes with launch keys: the leaves run in two
    launches, the resolution once, with z indexed by the call's vote index.  Grid certificates lie in
    both launches and one certificate of crafted votes lies astride vote 65,536."""
    dig, offs, pks, sigs, fam = tg.launches_call(oracle)
    m, nv = len(offs) - 1, int(offs[-1])
    got = _child(tmp_path, "launches", {"NWC_VERIFY_MAX_LAUNCH": str(tg.MAX_LAUNCH)}, tg.LAUNCH_SEEDS,
                 dig=dig, offs=offs, pks=pks, sigs=sigs)
    assert int(got["devices"][0]) == 1
    for i, seed in enumerate(tg.LAUNCH_SEEDS):
        ocert, obits = tg.expect_certs(oracle, dig, offs, pks, sigs, tg.zs_at(seed, np.arange(nv)), threads=16)
        diff = np.nonzero(_bits(got["cert"][i], m) != ocert)[0]
        assert len(diff) == 0, (seed, [(int(c), fam[c], int(offs[c])) for c in diff[:8]])
        assert (_bits(got["bad"][i], nv) == ~obits).all()
        assert ocert[np.array(fam) == "filler"].all()


def test_two_device_contexts(oracle, tmp_path):
    """NWC_VIRTUAL_DEVICES = 2 with the committee set: the host entry cuts the call on a certificate
    boundary (nwc_cert_cuts) and each context hashes vote indices local to its range."""
    from narwhal_amd import shard
    inst = tg.instance(oracle, "resolve", 63)
    cuts = shard.cert_cuts(inst.offs, 2)
    got = _child(tmp_path, "devices", {"NWC_VIRTUAL_DEVICES": "2"}, [tg.DEVICES_SEED], dig=inst.dig, offs=inst.offs,
                 pks=inst.pks, sigs=inst.sigs, committee=tg.committee(oracle, True))
    assert int(got["devices"][0]) == 2 and got["cuts"].tolist() == cuts and 0 < cuts[1] < inst.nv
    ocert, obits = tg.expected(oracle, inst, tg.DEVICES_SEED, False, tg.local_index(inst.nv, cuts), "local2")
    diff = np.nonzero(_bits(got["cert"][0], inst.m) != ocert)[0]
    assert len(diff) == 0, _names(inst, diff)
    assert (_bits(got["bad"][0], inst.nv) == ~obits).all()
