"""Subprocess body of tests/test_gpu_tables.py for the tables whose shape a process fixes at start
(NWC_COMB16, NWC_AUTO_KEYS are read once) or that need a library nobody else has used (the launch
keys): a fresh child per mode, which runs the checks of tests/table_audit.py itself -- a failed
check ends it with a traceback -- and writes what the parent asserts on as JSON.

  nocomb16   NWC_COMB16=0: comb16 is not built; base_table, comb_base and base24 are audited
  auto       NWC_AUTO_KEYS=20: 24 keys through two-key certificates, twice each, then a last round
  launch     three batch-leaf launches of 65,536 equations without a committee
"""
import ctypes
import json
import random
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[1])
from narwhal_amd import _lib, device  # noqa: E402
from oracle import ed25519_ref as ref  # noqa: E402
from tests import prim_probe as pp  # noqa: E402
from tests import table_audit as ta  # noqa: E402

mode, out_path = sys.argv[2], sys.argv[3]
pp.load()
lib = _lib.load()
B = ref.BASEPOINT


def keypairs(tag, n):
    seeds = device.derive32(tag, 0, n)
    msgs = device.derive32(tag + b"-msg", 0, n)
    pks, _ = device.keygen_sign(seeds, msgs)
    torch.cuda.synchronize()
    return seeds, [bytes(k) for k in pks.cpu().numpy()]


def nocomb16():
    digest = device.derive32(b"nocomb16", 0, 1)
    seeds, _ = keypairs(b"nocomb16-key", 1)
    pks, sigs = device.keygen_sign(seeds, digest)
    torch.cuda.synchronize()
    rc = lib.nwc_verify_strict(_lib.buf(digest.cpu().numpy()), _lib.buf(pks.cpu().numpy()), _lib.buf(sigs.cpu().numpy()))
    assert rc == 0, rc
    comb16, _ = pp.library_table("comb16")
    audited, exact = {}, 0
    tab, _ = pp.library_table("base_table")
    ta.check_entries(pp.gather(tab, np.arange(258)), ta.multiples(B, 0, 129) + ta.multiples(ref.pt_mul(1 << 132, B), 0, 129),
                     "base_table")
    ta.clean(tab, 2, 129, "base_table")
    audited["base_table"], exact = 258, exact + 258
    for name, windows, bits, bases in (("comb_base", 32, 8, ta.doublings(B, 8 * 31)[::8]),
                                       ("base24", 2, 24, [B, ref.pt_mul(1 << 141, B)])):
        tab, _ = pp.library_table(name)
        entries = (1 << (bits - 1)) + 1
        assert (tab.stride, tab.elements) == (128, windows * entries)
        ta.clean(tab, windows, entries, name)
        for w in range(windows):
            samples = ta.window_samples(ta.doublings(bases[w], bits - 1), entries, neighbours=False)
            ta.check_window(tab, w * entries, samples, "%s window %d" % (name, w))
            exact += len(samples)
        audited[name] = windows * entries
    return {"comb16": comb16, "audited": audited, "exact": exact}


def auto():
    from tests.oracle_lib import load_oracle
    oracle = load_oracle()
    n_keys = 24
    seeds, keys = keypairs(b"table-audit-auto", n_keys)
    digest = device.derive32(b"table-audit-auto-digest", 0, 1)
    pks, sigs = device.keygen_sign(seeds, digest.expand(n_keys, 32).contiguous())
    torch.cuda.synchronize()
    pks, sigs, dg = pks.cpu().numpy(), sigs.cpu().numpy(), digest.cpu().numpy().tobytes()
    assert [bytes(k) for k in pks] == keys

    def cert(pair, corrupt=None):
        p = np.ascontiguousarray(pks[list(pair)])
        s = np.ascontiguousarray(sigs[list(pair)]).copy()
        if corrupt is not None:
            s[corrupt, 40] ^= 1
        bad = ctypes.create_string_buffer(2)
        rc = lib.nwc_verify_batch(_lib.buf(dg), _lib.buf(p), _lib.buf(s), len(pair), bad)
        want = oracle.leaf_many(np.frombuffer(dg * len(pair), np.uint8).reshape(-1, 32), p, s)
        return [rc, bad.raw[0]], [0 if want.all() else 1, int(sum((not ok) << i for i, ok in enumerate(want)))]

    _lib.check(lib.nwc_set_committee(None, 0))
    pairs = [(2 * i, 2 * i + 1) for i in range(n_keys // 2)]
    for sight in range(2):                                      # the second sight of a key adds it
        for pair in pairs:
            got, want = cert(pair)
            assert got == want == [0, 0], (sight, pair, got, want)
    cap = ctypes.c_uint32()
    _lib.check(lib.nwc_auto_cache_info(ctypes.byref(cap), None, None))
    held_arr, held = pp.library_table("auto_keys")
    assert held == 20, held
    held_keys = [k.astype("<u4").tobytes() for k in pp.read_array(held_arr)]
    order = [keys.index(k) for k in held_keys]
    ta.check_key_arrays("auto", held_keys, random.Random(2001))
    verdicts, oracle_says = [], []
    for i, pair in enumerate(pairs):                            # held keys: the latency kernel; replaced ones: uncached
        got, want = cert(pair, corrupt=(i % 2 if i % 3 == 0 else None))
        verdicts.append(got)
        oracle_says.append(want)
    return {"held": order, "capacity": cap.value, "checked_keys": len(held_keys), "verdicts": verdicts, "oracle": oracle_says}


def launch():
    n = 65536
    seeds, keys = keypairs(b"table-audit-launch", 12)
    msgs = device.derive32(b"table-audit-launch-msg", 0, n)
    rng = np.random.default_rng(5)
    _lib.check(lib.nwc_set_committee(None, 0))
    log = []
    for who in (range(6), range(12), range(12)):
        pick = torch.from_numpy(rng.integers(who.start, who.stop, n)).cuda()
        pks, sigs = device.keygen_sign(seeds[pick].contiguous(), msgs)
        corrupt = torch.from_numpy(rng.random(n) < 0.01).cuda()
        sigs[corrupt, 40] ^= 1
        words = device.verify(msgs, pks, sigs, strict=False)
        torch.cuda.synchronize()
        got = device.unpack_bits(words, n)
        held_arr, held = pp.library_table("launch_keys")
        held_keys = [k.astype("<u4").tobytes() for k in pp.read_array(held_arr)]
        assert len(held_keys) == held and set(held_keys) <= set(keys[:who.stop])
        ta.check_key_arrays("launch", held_keys, random.Random(3001 + len(log)), tables=False)
        log.append({"held": held, "keys": [k.hex() for k in held_keys], "checked_keys": len(held_keys),
                    "verdicts_ok": bool((got == ~corrupt.cpu().numpy()).all())})
    _lib.check(lib.nwc_set_committee(None, 0))
    return {"launches": log, "expected_keys": [k.hex() for k in keys]}


result = {"nocomb16": nocomb16, "auto": auto, "launch": launch}[mode]()
json.dump(result, open(out_path, "w"))
print("table_audit_helper %s: ok" % mode)
