"""Builders and expectations of the torsion-grid tests (tests/test_gpu_torsion_grid.py,
tests/test_torsion_grid_host.py): plain numpy, hashlib and the CPU oracle, no device code.

tests/golden/torsion_grid.json holds one vote for every cell (a, b) of E[8] x E[8]: residual
e = [a] G8, key with l A = [b] G8, all over one message (tests/golden/make_torsion_grid.py).  From
them this module builds the calls the GPU tests make -- certificates for the per-certificate
resolution (narwhal_amd/csrc/resolve.h), 64-vote groups for the Pippenger kernel (msm.h), 8-vote
sub-batches for the Straus kernel (straus.h) -- and says what dalek's equation answers on each for the
z_i a fixed `dalek_seed` gives: the oracle's term-by-term evaluation (orc_batch_z_many, z8 = False),
never the device's own arithmetic.  It also holds the rows and the checkers of the probe entries for
torsion_dlog, ge_mul_l, straus_z, sc_mul128 and resolve_q8 (tests/hip/grid_probe.hip).
"""
from __future__ import annotations

import functools
import hashlib
import json
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import ed25519_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_JSON = os.path.join(ROOT, "tests", "golden", "torsion_grid.json")
P, L = ref.P, ref.L

# The seeds the GPU tests fix (nwc_diag_set("dalek_seed")).  tests/test_torsion_grid_host.py asserts
# that, for each, the oracle alone accepts and rejects at least four certificates (groups) of every
# randomized family below: a seed under which all of them fail (or pass) would pin little.
SEEDS = (11, 12, 13, 14, 15)
HOST_ENTRY_SEED = 21
LAUNCH_SEEDS = (12, 14)
DEVICES_SEED = 13
TAILS = (0, 1, 63)          # nv % 64 of the resolve instance: the last word of k_list_failing
MSM_GROUP, MSM_GROUPS = 64, 64
STRAUS_NQ, STRAUS_RUNS = 8, 128
MAX_LAUNCH = 65536


# ---- the fixture --------------------------------------------------------------------------------
class Grid:
    def __init__(self, doc):
        self.msg = np.frombuffer(bytes.fromhex(doc["msg"]), np.uint8).copy()
        self.keys = np.frombuffer(b"".join(bytes.fromhex(k) for k in doc["keys"]), np.uint8).reshape(8, 32).copy()
        self.pk = np.zeros((8, 8, 32), np.uint8)      # [a][b]
        self.sig = np.zeros((8, 8, 64), np.uint8)
        seen = set()
        for v in doc["votes"]:
            a, b = v["a"], v["b"]
            seen.add((a, b))
            self.pk[a, b] = np.frombuffer(bytes.fromhex(v["pk"]), np.uint8)
            self.sig[a, b] = np.frombuffer(bytes.fromhex(v["sig"]), np.uint8)
        assert seen == {(a, b) for a in range(8) for b in range(8)} and len(doc["votes"]) == 64
        assert all((self.pk[a, b] == self.keys[b]).all() for a in range(8) for b in range(8))
        self.filler_seeds = np.frombuffer(b"".join(bytes.fromhex(s) for s in doc["filler_seeds"]), np.uint8).reshape(-1, 32).copy()


@functools.lru_cache(maxsize=None)
def load_grid() -> Grid:
    with open(GRID_JSON) as f:
        return Grid(json.load(f))


@functools.lru_cache(maxsize=None)
def undecodable_key() -> bytes:
    """The smallest y >= 2 that is no point's y: a key that fails decompression."""
    y = 2
    while ref.decompress(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


_FILLERS = {}


def fillers(oracle):
    """(pks, sigs): the honest votes of the filler keys over the grid's message."""
    if "v" not in _FILLERS:
        g = load_grid()
        n = len(g.filler_seeds)
        _FILLERS["v"] = oracle.keygen_sign_many(g.filler_seeds, np.tile(g.msg, (n, 1)))
    return _FILLERS["v"]


# ---- votes, certificates, instances -------------------------------------------------------------
# A vote is ("cell", a, b): the grid's crafted vote; ("honest", f): filler key f's vote over msg;
# ("flip", a, b): the crafted vote with one s byte flipped (a prime-order residual: deterministic Err);
# ("nokey", f): filler f's signature under the undecodable key (deterministic Err).
def _vote_bytes(oracle, vote):
    g = load_grid()
    fp, fs = fillers(oracle)
    kind = vote[0]
    if kind == "cell":
        return g.pk[vote[1], vote[2]], g.sig[vote[1], vote[2]]
    if kind == "honest":
        return fp[vote[1] % len(fp)], fs[vote[1] % len(fs)]
    if kind == "flip":
        s = g.sig[vote[1], vote[2]].copy()
        s[33] ^= 1
        return g.pk[vote[1], vote[2]], s
    assert kind == "nokey"
    return np.frombuffer(undecodable_key(), np.uint8), fs[vote[1] % len(fs)]


def crafted(vote) -> bool:
    return vote[0] == "cell" and (vote[1], vote[2]) != (0, 0)


class Instance:
    """certs: a list of (family, [votes]); every certificate's digest is the grid's message."""

    def __init__(self, oracle, certs):
        self.families = [f for f, _ in certs]
        self.votes = [v for _, vs in certs for v in vs]
        sizes = [len(vs) for _, vs in certs]
        self.offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.m, self.nv = len(certs), int(self.offs[-1])
        g = load_grid()
        self.dig = np.tile(g.msg, (self.m, 1))
        pairs = [_vote_bytes(oracle, v) for v in self.votes]
        self.pks = np.ascontiguousarray(np.stack([p for p, _ in pairs]))
        self.sigs = np.ascontiguousarray(np.stack([s for _, s in pairs]))
        self.crafted = np.array([crafted(v) for v in self.votes])

    def of_family(self, *families):
        return [c for c, f in enumerate(self.families) if f in families]


def _honest(rng, n):
    return [("honest", rng.randrange(1 << 16)) for _ in range(n)]


def _mixed(rng, votes, honest):
    """`votes` and `honest` honest ones, shuffled."""
    out = list(votes) + _honest(rng, honest)
    rng.shuffle(out)
    return out


def _cells(rng, n):
    """n crafted cells (never the honest cell (0, 0)), repeats allowed."""
    out = []
    while len(out) < n:
        a, b = rng.randrange(8), rng.randrange(8)
        if (a, b) != (0, 0):
            out.append(("cell", a, b))
    return out


def resolve_certs(tail: int):
    """The certificates of the per-certificate resolution's instance, nv % 64 == tail:
      single   all 64 cells alone, one per certificate, between honest votes (cell (0, 0): all honest)
      multi    32 certificates each of 2, 3, 5 and 8 crafted votes drawn across the cells
      onekey   16 certificates whose crafted votes all come from one torsion-bearing key: for every b all
               eight cells (a, b), and three of them
      err      8 certificates of crafted votes and one deterministic failure (RESOLVE_ERR beside torsion)
      wide     2 certificates of 300 crafted votes (several waves and blocks of k_vote_resolve, hundreds of
               atomicAdd into one cert_state word)
      pad      one honest certificate sized to give the tail
    The call's first and last votes are crafted."""
    rng = random.Random(1000 + tail)
    certs = []
    for b in range(8):
        for a in range(8):
            vs = [("cell", a, b)] + _honest(rng, 2)
            if certs:
                rng.shuffle(vs)
            certs.append(("single", vs))
    assert certs[0][1][0] == ("cell", 0, 0)
    certs[0], certs[1] = certs[1], certs[0]
    certs[0] = ("single", [("cell", 1, 0)] + _honest(rng, 2))     # the call's first vote is crafted
    for n in (2, 3, 5, 8):
        for _ in range(32):
            certs.append(("multi", _mixed(rng, _cells(rng, n), rng.randrange(0, 4))))
    for b in range(8):
        certs.append(("onekey", _mixed(rng, [("cell", a, b) for a in range(8) if (a, b) != (0, 0)], 2)))
        certs.append(("onekey", _mixed(rng, [("cell", a, b) for a in rng.sample(range(1, 8), 3)], 1)))
    for i in range(8):
        bad = ("flip", rng.randrange(8), rng.randrange(8)) if i % 2 == 0 else ("nokey", i)
        certs.append(("err", _mixed(rng, _cells(rng, 1 + i % 3) + [bad], 2)))
    wides = [("wide", _cells(rng, 300)) for _ in range(2)]
    certs.insert(40, wides[0])
    nv = sum(len(vs) for _, vs in certs) + 300
    pad = (tail - nv) % 64
    if pad:
        certs.append(("pad", _honest(rng, pad)))
    certs.append(wides[1])                                         # and its last vote
    assert sum(len(vs) for _, vs in certs) % 64 == tail
    assert crafted(certs[0][1][0]) and crafted(certs[-1][1][-1])
    return certs


def _group_design(rng, groups: int, size: int, max_few: int):
    """`groups` groups of `size` consecutive votes (Pippenger groups, Straus sub-batches): a quarter all
    honest, groups with 1..max_few crafted votes, at least twelve where one torsion-bearing key signs two
    or more crafted votes, two with a deterministic failure beside crafted votes and four all crafted;
    the first and the last vote of the call are crafted."""
    out = []
    for b in list(range(1, 8)) + [1, 3, 5, 7, 2]:
        n = min(size, rng.randrange(2, 9))
        out.append(("onekey", _mixed(rng, [("cell", a, b) for a in rng.sample(range(8), n)], size - n)))
    for i in range(2):
        out.append(("err", _mixed(rng, _cells(rng, 2) + [("flip", 3, i)], size - 3)))
    for _ in range(4):
        out.append(("crafted", _cells(rng, size)))
    for _ in range(groups // 4):
        out.append(("honest", _honest(rng, size)))
    while len(out) < groups:
        n = rng.randrange(1, max_few + 1)
        out.append(("few", _mixed(rng, _cells(rng, n), size - n)))
    rng.shuffle(out)
    first = next(i for i, (f, _) in enumerate(out) if f == "crafted")
    out[0], out[first] = out[first], out[0]
    last = next(i for i, (f, _) in enumerate(out) if f == "crafted" and i != 0)
    out[-1], out[last] = out[last], out[-1]
    assert all(len(vs) == size for _, vs in out) and len(out) == groups
    return out


def msm_groups():
    return _group_design(random.Random(2064), MSM_GROUPS, MSM_GROUP, 4)


def straus_groups():
    return _group_design(random.Random(2008), STRAUS_RUNS, STRAUS_NQ, 3)


_INSTANCES = {}


def instance(oracle, name, *args) -> Instance:
    """resolve (tail), msm, straus: built once per process."""
    key = (name,) + args
    if key not in _INSTANCES:
        certs = {"resolve": resolve_certs, "msm": msm_groups, "straus": straus_groups}[name](*args)
        _INSTANCES[key] = Instance(oracle, certs)
    return _INSTANCES[key]


def committee(oracle, grid_keys: bool) -> np.ndarray:
    """The filler keys, with the eight grid keys (the comb inside the resolution) or without them (the
    grid's votes take the ladder, in the same waves as the fillers' comb)."""
    fp, _ = fillers(oracle)
    keys = [fp] + ([load_grid().keys] if grid_keys else [])
    return np.ascontiguousarray(np.unique(np.concatenate(keys), axis=0))


# ---- z_i and dalek's equation -------------------------------------------------------------------
def seed_bytes(seed: int) -> bytes:
    """draw_seed (nwc_api.hip): the knob's low 32 bits in word 0, zeros after."""
    return (seed & 0xFFFFFFFF).to_bytes(4, "little") + bytes(28)


def zs_at(seed: int, index) -> np.ndarray:
    """z of every vote, (nv, 16) bytes: SHA-512(seed || u64le(index[v]))[..16] (straus_z).  `index` maps a
    vote to the index the kernel hashes: the call's (np.arange(nv)), or local to a range."""
    sb = seed_bytes(seed)
    idx = np.asarray(index, dtype=np.int64)
    return np.frombuffer(b"".join(hashlib.sha512(sb + int(v).to_bytes(8, "little")).digest()[:16] for v in idx),
                         np.uint8).reshape(len(idx), 16)


def local_index(nv: int, cuts) -> np.ndarray:
    """Vote index local to its range [cuts[i], cuts[i + 1])."""
    idx = np.arange(nv, dtype=np.int64)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        idx[lo:hi] -= lo
    return idx


def equation(oracle, dig, offs, pks, sigs, zs, z8: bool = False, threads: int = 8) -> np.ndarray:
    """orc_batch_z_many over the certificates [offs[c], offs[c + 1]), a slice of them per thread (the
    oracle's entry is single-threaded and the term-by-term form costs ~0.3 ms a vote)."""
    offs = np.asarray(offs, dtype=np.int64)
    m = len(offs) - 1
    if m == 0:
        return np.zeros(0, bool)
    bounds = sorted({int(np.searchsorted(offs, offs[-1] * t // threads, side="left")) for t in range(threads)} | {0, m})
    bounds = [b for b in bounds if b <= m]

    def part(i):
        c0, c1 = bounds[i], bounds[i + 1]
        v0, v1 = int(offs[c0]), int(offs[c1])
        return oracle.batch_z_many(np.ascontiguousarray(dig[c0:c1]), (offs[c0:c1 + 1] - v0).astype(np.uint32),
                                   np.ascontiguousarray(pks[v0:v1]), np.ascontiguousarray(sigs[v0:v1]),
                                   np.ascontiguousarray(zs[v0:v1]), z8=z8)
    with ThreadPoolExecutor(threads) as ex:
        return np.concatenate(list(ex.map(part, range(len(bounds) - 1))))


def leaves(oracle, dig, offs, pks, sigs) -> np.ndarray:
    return oracle.leaf_many(np.ascontiguousarray(np.repeat(dig, np.diff(offs), axis=0)), pks, sigs).astype(bool)


def expect_certs(oracle, dig, offs, pks, sigs, zs, z8: bool = False, threads: int = 8):
    """Per certificate (the resolution): cert_ok[c] = dalek's equation over certificate c's votes with
    these z; leaf bit v = leaf_ok(v) or cert_ok[cert(v)].  Returns (cert_ok, leaf bits)."""
    cert = equation(oracle, dig, offs, pks, sigs, zs, z8, threads)
    bits = leaves(oracle, dig, offs, pks, sigs) | np.repeat(cert, np.diff(offs))
    return cert, bits


def expect_groups(oracle, msg, cuts, pks, sigs, zs, z8: bool = False):
    """Per group of consecutive votes [cuts[g], cuts[g + 1]) (Pippenger groups, Straus sub-batches), every
    vote over `msg`: group_ok[g] = the equation over the group taken as one certificate; leaf bit v =
    leaf_ok(v) or group_ok[g(v)] (a group that fails hands its votes to the exact leaves)."""
    cuts = np.asarray(cuts, dtype=np.int64)
    return expect_certs(oracle, np.tile(msg, (len(cuts) - 1, 1)), cuts, pks, sigs, zs, z8)


_EXPECTED = {}


def expected(oracle, inst: Instance, seed: int, z8: bool = False, index=None, tag="call"):
    """expect_certs of an instance for a seed, computed once (the GPU tests of both resolve branches and
    the host tests share it)."""
    key = (id(inst), seed, z8, tag)
    if key not in _EXPECTED:
        idx = np.arange(inst.nv) if index is None else index
        _EXPECTED[key] = expect_certs(oracle, inst.dig, inst.offs, inst.pks, inst.sigs, zs_at(seed, idx), z8)
    return _EXPECTED[key]


# ---- the equation in Python, and the mutation the repeated-key groups must see ------------------
def python_equation(msg: bytes, votes, zs):
    """dalek's equation as msm.h arranges it: -(sum z_i s_i mod l) B + sum z_i R_i + sum_j c_j A_j, c_j the
    sum over key j's votes of (z_i k_i mod l).  Returns (verdict, mutated verdict): dalek's own
    coefficients are kept when c_j stays unreduced; the mutation takes c_j mod l -- the bug: it shifts
    the result by a multiple of l A_j, which is no identity for a torsion-bearing key."""
    bcoef, acc, sums = 0, ref.IDENTITY, {}
    for (pk, sig), z in zip(votes, zs):
        if not ref.sig_scalar_ok(sig):
            return False, False
        A, R = ref.decompress(pk), ref.decompress(sig[:32])
        if A is None or R is None:
            return False, False
        k = ref.scalar_from_hash(ref.sha512(sig[:32] + pk + msg))
        bcoef = (bcoef + z * int.from_bytes(sig[32:], "little")) % L
        acc = ref.pt_add(acc, ref.pt_mul(z, R))
        sums[pk] = sums.get(pk, 0) + z * k % L
    acc = ref.pt_add(acc, ref.pt_mul((-bcoef) % L, ref.BASEPOINT))
    exact = mutated = acc
    for pk, c in sums.items():
        A = ref.decompress(pk)
        exact = ref.pt_add(exact, ref.pt_mul(c, A))
        mutated = ref.pt_add(mutated, ref.pt_mul(c % L, A))
    return exact == ref.IDENTITY, mutated == ref.IDENTITY


# ---- the Straus cut -----------------------------------------------------------------------------
def straus_constants():
    """STRAUS_MAX_PER_LANE and NWC_STRAUS_WAVES_PER_SIMD as straus.h states them."""
    src = open(os.path.join(ROOT, "narwhal_amd", "csrc", "straus.h")).read()
    return (int(re.search(r"constexpr int STRAUS_MAX_PER_LANE = (\d+);", src).group(1)),
            int(re.search(r"#define NWC_STRAUS_WAVES_PER_SIMD (\d+)", src).group(1)))


def straus_runs(nv: int, lanes: int, target: int, max_per_lane: int = 16) -> int:
    """straus_runs (straus.h), line for line."""
    target = min(max(target, 1), max_per_lane)
    want = (nv + target - 1) // target
    if want <= lanes:
        return want
    rounds = max((want + lanes // 2) // lanes, 1)
    while (nv + rounds * lanes - 1) // (rounds * lanes) > max_per_lane:
        rounds += 1
    return rounds * lanes


def straus_cuts(nv: int, runs: int):
    """Sub-batch r = votes [r nv / runs, (r + 1) nv / runs) (k_verify_straus)."""
    return [r * nv // runs for r in range(runs + 1)]


# ---- the several-launches call ------------------------------------------------------------------
def launches_call(oracle):
    """A call of more than MAX_LAUNCH votes (launch keys; the leaves run in two launches, the resolution
    once over the whole call): grid certificates, honest 67-vote certificates of a 100-key committee,
    one certificate over the grid's message that straddles vote MAX_LAUNCH with crafted votes on both
    sides, more honest certificates, grid certificates.  Returns (dig, offs, pks, sigs, families)."""
    front = resolve_certs(1)[:70]
    back = resolve_certs(63)[70:140] + [("multi", [("honest", 7), ("cell", 3, 5), ("cell", 2, 7)])]
    straddle = [("cell", 1 + i % 7, (i // 7) % 8) if i % 5 == 0 else ("honest", i) for i in range(140)]
    fi, bi = Instance(oracle, front), Instance(oracle, back)
    si = Instance(oracle, [("straddle", straddle)])
    before = (MAX_LAUNCH - 40 - fi.nv) // 67
    after = 40
    nrng = np.random.default_rng(67)
    kseeds = nrng.integers(0, 256, (100, 32), dtype=np.uint8)
    hdig = nrng.integers(0, 256, (before + after, 32), dtype=np.uint8)
    who = np.concatenate([nrng.permutation(100)[:67] for _ in range(before + after)])
    hp_, hs = oracle.keygen_sign_many(kseeds[who], np.repeat(hdig, 67, axis=0))
    cut = 67 * before
    dig = np.concatenate([fi.dig, hdig[:before], si.dig, hdig[before:], bi.dig])
    pks = np.concatenate([fi.pks, hp_[:cut], si.pks, hp_[cut:], bi.pks])
    sigs = np.concatenate([fi.sigs, hs[:cut], si.sigs, hs[cut:], bi.sigs])
    sizes = list(np.diff(fi.offs)) + [67] * before + [140] + [67] * after + list(np.diff(bi.offs))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    families = fi.families + ["filler"] * before + ["straddle"] + ["filler"] * after + bi.families
    craft = np.concatenate([fi.crafted, np.zeros(cut, bool), si.crafted, np.zeros(67 * after, bool), bi.crafted])
    s0 = fi.nv + cut
    assert s0 < MAX_LAUNCH < s0 + 140 and craft[s0:MAX_LAUNCH].any() and craft[MAX_LAUNCH:s0 + 140].any()
    assert MAX_LAUNCH < int(offs[-1]) < 2 * MAX_LAUNCH and craft[0] and craft[-1]
    return (np.ascontiguousarray(dig), offs, np.ascontiguousarray(pks), np.ascontiguousarray(sigs), families)


# ---- probe rows and checkers --------------------------------------------------------------------
def _g8():
    return ref.decompress(bytes.fromhex(ref.G8_HEX))


def torsion_points():
    return [ref.pt_mul(j, _g8()) for j in range(8)]


def _forms(x: int, form: int):
    """10 signed limbs of x mod p in one of three forms, all within the loose bound of fe_mul's inputs:
    0 tight and centred (what the kernel hands torsion_dlog), 1 the non-negative limbs of the canonical
    value, 2 the centred limbs plus the limbs of p (the non-canonical value x + p)."""
    from tests import prim_probe as pp
    if form == 0:
        return pp.centred_limbs(x)
    if form == 1:
        return pp.limbs_of(x % P)
    return [c + q for c, q in zip(pp.centred_limbs(x), pp.limbs_of(P))]


def dlog_rows(seed: int = 8):
    """(records (N, 30) int32, expected (N,)): every torsion point in the three limb forms with Z = 1,
    random Z, Z = -1 and Z = 2 (expected j), and points outside E[8] -- n B + T[j], 2^k B, a torsion point
    with one coordinate off by one -- (expected 8)."""
    rng = random.Random(seed)
    T = torsion_points()
    rows, want = [], []

    def add(pt, z, form, j):
        x, y = pt
        rows.append(_forms(x * z % P, form) + _forms(y * z % P, form) + _forms(z, form))
        want.append(j)
    for j, pt in enumerate(T):
        for form in range(3):
            for z in [1, P - 1, 2] + [rng.randrange(2, P) for _ in range(7)]:
                add(pt, z, form, j)
    for i in range(40):
        n = rng.randrange(1, L)
        add(ref.pt_add(ref.pt_mul(n, ref.BASEPOINT), T[i % 8]), rng.randrange(1, P), i % 3, 8)
    for k in range(8):
        add(ref.pt_mul(1 << k, ref.BASEPOINT), 1, 0, 8)
    for j, (x, y) in enumerate(T):     # off the curve, next to a torsion point: still not one of the eight
        add(((x + 1) % P, y), rng.randrange(1, P), 0, 8)
        add((x, (y + 1) % P), 1, 1, 8)
    rec = np.array(rows, dtype=np.int64).astype(np.int32)
    return rec, np.array(want, dtype=np.uint32)


def check_dlog(out, want):
    got = np.asarray(out).reshape(-1)
    assert got.shape == np.asarray(want).shape
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "torsion_dlog: record %d gives %d, expected %d" % (bad[0], got[bad[0]], want[bad[0]])


def mul_l_rows(seed: int = 9):
    """(records (N, 8) words, expected dlog, expected decode flag): P = n B + T[j] for every j and several n
    (l P = [5 j mod 8] G8), the small-order points themselves (n = 0, the identity among them), their
    second encodings with the sign bit of x = 0 set, and the undecodable key (flag 0; its dlog is not read)."""
    rng = random.Random(seed)
    T = torsion_points()
    encs, want, flag = [], [], []
    nB = [ref.pt_mul(n, ref.BASEPOINT) for n in [0, 1, 2, L - 1, 8] + [rng.randrange(1, L) for _ in range(28)]]
    for j in range(8):
        for Q in nB:
            encs.append(ref.compress(ref.pt_add(Q, T[j])))
            want.append(5 * j % 8)
            flag.append(1)
    for j in (0, 4):                 # x = 0: the encoding with the sign bit set decodes to the same point
        e = bytearray(ref.compress(T[j]))
        e[31] |= 0x80
        encs.append(bytes(e))
        want.append(5 * j % 8)
        flag.append(1)
    encs.append(undecodable_key())
    want.append(0)
    flag.append(0)
    rec = np.frombuffer(b"".join(encs), np.uint8).reshape(-1, 32).view("<u4").astype(np.uint32)
    return rec, np.array(want, np.uint32), np.array(flag, np.uint32)


def check_mul_l(out, want, flag):
    out = np.asarray(out)
    assert out.shape == (len(want), 2)
    bad = np.nonzero(out[:, 1] != flag)[0]
    assert len(bad) == 0, "ge_mul_l probe: record %d decodes = %d, expected %d" % (bad[0], out[bad[0], 1], flag[bad[0]])
    bad = np.nonzero((out[:, 0] != want) & (flag == 1))[0]
    assert len(bad) == 0, "ge_mul_l: record %d gives dlog %d, expected %d" % (bad[0], out[bad[0], 0], want[bad[0]])


def zq_rows(seed: int = 10):
    """(records (N, 18) words, [(seed bytes, v, k)]): random seeds, v and k < 2^256 wide; v at 0, 2^32 - 1,
    2^32, 2^63 and 2^64 - 1; k at 0, 1, l - 1, l, 2^256 - 1 and 2^252 (sc_mul128 takes any 256-bit k)."""
    rng = random.Random(seed)
    cases = []
    vs = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, 1 << 63, (1 << 64) - 1]
    ks = [0, 1, L - 1, L, L + 1, (1 << 256) - 1, 1 << 252, 8 * L - 1]
    for v in vs:
        for k in ks[:4]:
            cases.append((seed_bytes(rng.choice(SEEDS)), v, k))
    for k in ks:
        cases.append((rng.randbytes(32), rng.getrandbits(64), k))
    for _ in range(300):
        cases.append((rng.randbytes(32) if rng.random() < 0.5 else seed_bytes(rng.randrange(1, 1 << 32)),
                      rng.getrandbits(rng.choice((8, 20, 33, 64))), rng.randrange(L)))
    rec = np.array([list(np.frombuffer(s, "<u4")) + [v & 0xFFFFFFFF, v >> 32] + [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
                    for s, v, k in cases], dtype=np.uint32)
    return rec, cases


def zq_direct_rows(seed: int = 11):
    """(records (N, 12) words, [(z, k)]): z at 0, 1, 7, 8, 2^128 - 1 and random against k at 0, 1, l - 1, l,
    2^256 - 1 and random."""
    rng = random.Random(seed)
    zs = [0, 1, 7, 8, (1 << 128) - 1, (1 << 128) - 8, 1 << 127] + [rng.getrandbits(128) for _ in range(12)]
    ks = [0, 1, L - 1, L, (1 << 256) - 1, L - 8] + [rng.randrange(L) for _ in range(12)]
    cases = [(z, k) for z in zs for k in ks]
    rec = np.array([[(z >> (32 * i)) & 0xFFFFFFFF for i in range(4)] + [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
                    for z, k in cases], dtype=np.uint32)
    return rec, cases


def _words(row) -> int:
    return sum(int(w) << (32 * i) for i, w in enumerate(row))


def check_zq_record(out_row, z_want: int, k: int, what: str = ""):
    """One record of probe_zq / probe_zq_direct: z, z k mod l and q8 = floor(z k / l) mod 8, on integers."""
    z, zk, q8 = _words(out_row[0:4]), _words(out_row[4:12]), int(out_row[12])
    assert z == z_want, "%s: z = %#x, expected %#x" % (what, z, z_want)
    assert zk == z * k % L, "%s: z k mod l = %#x, expected %#x" % (what, zk, z * k % L)
    assert q8 == (z * k // L) % 8, "%s: q8 = %d, expected %d" % (what, q8, (z * k // L) % 8)


def check_zq(out, cases):
    assert len(out) == len(cases)
    for i, (row, (s, v, k)) in enumerate(zip(out, cases)):
        z = int.from_bytes(hashlib.sha512(s + v.to_bytes(8, "little")).digest()[:16], "little")
        check_zq_record(row, z, k, "probe_zq record %d" % i)


def check_zq_direct(out, cases):
    assert len(out) == len(cases)
    for i, (row, (z, k)) in enumerate(zip(out, cases)):
        check_zq_record(row, z, k, "probe_zq_direct record %d" % i)
