"""Fixtures and child processes of tests/test_gpu_sanitize_ex.py (nwc_sanitize_messages_ex,
nwc_dev_sanitize_messages_ex).

Imported, it gives the committee (four single-stake keys and one key without stake), the wire
messages built with oracle/messages_ref.py's encoders, and the ctypes callers.  Run as a program it
is a child process, because libnwc reads its environment once per process:

  chunked       NWC_MSG_CHUNK=1048576 in the environment: the fixture messages tiled to just over
                4 MiB, so the call is staged and cut; the first and last message of every chunk under
                a state that differs from their neighbours'; twice on the same stages; against the
                same batch in calls of at most 1 MiB
  wrong_device  NWC_VIRTUAL_DEVICES=2: a signer on context 1 with a device call on context 0, a
                host call that carries it, and a call without a signer sharded over both contexts
  memory        a process that only calls _ex without a signer builds no signing table

usage: sanitize_ex_helper.py MODE ROOT; prints one JSON line."""
import base64
import bisect
import ctypes
import json
import os
import struct
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[2])
    sys.path.insert(0, os.path.join(sys.argv[2], "oracle"))

from tests.test_gpu_messages import _install  # noqa: E402
from tests.test_gpu_sanitizer import _World  # noqa: E402

SIGNER_KEY = 1      # the signer's key is the committee's second
STALE_GC = 1000     # above every fixture round: headers and certificates are TooOld under it


class ExWorld(_World):
    """Four single-stake authorities and a fifth key without stake."""

    def __init__(self, oracle, seed=77):
        super().__init__(oracle, 5, seed)
        self.committee = self.mr.RefCommittee({pk: ((1 if k < 4 else 0), [0]) for k, pk in enumerate(self.pks)})

    def install(self, lib):
        _install(lib, self.pks, [1, 1, 1, 1, 0], [[0]] * 5)

    def header_with(self, k, rnd, nparents, hid=None, author_text=None, flip_sig=False):
        parents = [self.rand32() for _ in range(nparents)]
        true_id = self.mr.header_id(self.pks[k], rnd, [], parents)
        hid = true_id if hid is None else hid
        sig = self.o.sign(self.seeds[k], hid)
        if flip_sig:
            sig = sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]
        return self.mr.msg_header(self.mr.enc_header(self.pks[k], rnd, [], parents, hid, sig, author_text=author_text)), hid


def target_record(target):
    """The 80-byte record: id, round LE, origin, the "enabled" byte, seven zero bytes."""
    if target is None:
        return bytes(80)
    return target[0] + struct.pack("<Q", target[1]) + target[2] + b"\x01" + bytes(7)


def fixture(w):
    """name -> (wire message, gc_round, vote target or None), the state under which the message is
    judged in the tests.  Every header has round 5, every vote and certificate round 7 or 3."""
    mr = w.mr
    f = {}
    f["hdr-ok"] = (w.header_with(0, 5, 3)[0], 0, None)
    f["hdr-bad-sig"] = (w.header_with(2, 5, 2, flip_sig=True)[0], 0, None)
    f["hdr-bad-id"] = (w.header_with(3, 5, 2, hid=w.rand32())[0], 0, None)
    f["hdr-too-old"] = (w.header_with(0, 5, 1)[0], 6, None)
    f["hdr-at-gc"] = (f["hdr-too-old"][0], 5, None)            # the same header on the other side of its round
    # 36 bytes of key text: 48 symbols, no padding; the key is the first 32 bytes, and the round
    # sits 4 bytes further on than behind a 44-symbol key
    long_text = base64.b64encode(w.pks[3] + b"\x01\x02\x03\x04")
    assert len(long_text) == 48
    f["hdr-long-key"] = (w.header_with(3, 5, 2, author_text=long_text)[0], 2, None)
    f["hdr-no-stake"] = (w.header_with(4, 5, 1)[0], 0, None)
    hid, origin = w.rand32(), w.pks[1]
    vote = w.vote(2, hid, 7, origin)
    f["vote-ok"] = (vote, 0, (hid, 7, origin))
    f["vote-stale-target"] = (vote, 0, (w.rand32(), 7, origin))
    f["vote-no-target"] = (vote, 9, None)
    f["vote-old"] = (vote, 0, (hid, 8, origin))
    f["cert-ok"] = (w.certificate(1, 3, [0, 1, 2]), 3, None)
    f["cert-too-old"] = (f["cert-ok"][0], 4, None)
    f["cert-bad-vote"] = (w.certificate(2, 3, [0, 1, 3], bad_vote=1), 0, None)
    f["request"] = (struct.pack("<I", 3) + struct.pack("<Q", 1) + w.rand32() + mr.enc_key(w.pks[0]), 0, (hid, 7, origin))
    f["truncated"] = (f["hdr-ok"][0][:-10], 0, None)
    f["empty"] = (b"", 0, None)
    f["hdr-ok-last"] = (w.header_with(1, 5, 0)[0], 5, (hid, 7, origin))
    return f


EXPECTED_CODES = {"hdr-ok": 0, "hdr-bad-sig": 1, "hdr-bad-id": 2, "hdr-too-old": 7, "hdr-at-gc": 0, "hdr-long-key": 0,
                  "hdr-no-stake": 4, "vote-ok": 0, "vote-stale-target": 9, "vote-no-target": 0, "vote-old": 7, "cert-ok": 0,
                  "cert-too-old": 7, "cert-bad-vote": 1, "request": 10, "truncated": 8, "empty": 8, "hdr-ok-last": 0}


def pack(items):
    """items: (msg, gc_round, target) -> data, offsets, gc_rounds, target records"""
    m = len(items)
    offs = np.zeros(m + 1, np.uint64)
    offs[1:] = np.cumsum([len(it[0]) for it in items])
    data = np.frombuffer(b"".join(it[0] for it in items) or b"\0", np.uint8).copy()
    gcs = np.array([it[1] for it in items], np.uint64)
    tg = np.frombuffer(b"".join(target_record(it[2]) for it in items), np.uint8).reshape(m, 80).copy()
    return data, offs, gcs, tg


def run_ex(lib, items, signer=None, own_state=True, gc_round=0, target=None, digests=True):
    """nwc_sanitize_messages_ex over the items -> (codes, digests, kinds, vote_sigs, voted); the vote
    outputs start as 0xEE so that every byte the call leaves unwritten shows.  own_state: True (both
    arrays), False (neither: gc_round and target hold for every message), "gc" or "targets" (that
    array alone)."""
    from narwhal_amd import _lib
    data, offs, gcs, tg = pack(items)
    m = len(items)
    codes = np.full(m, -99, np.int32)
    dig = np.full((m, 32), 0xEE, np.uint8)
    kinds = np.full(m, 0xEE, np.uint8)
    sigs = np.full((m, 64), 0xEE, np.uint8)
    voted = np.full(m, 0xEE, np.uint8)
    tb = None if target is None else target[0] + struct.pack("<Q", target[1]) + target[2]
    _lib.check(lib.nwc_sanitize_messages_ex(_lib.buf(data), _lib.buf(offs), m, _lib.buf(gcs) if own_state in (True, "gc") else None,
                                            gc_round, _lib.buf(tg) if own_state in (True, "targets") else None, _lib.buf(tb) if tb else None, signer,
                                            _lib.buf(codes), _lib.buf(dig) if digests else None, _lib.buf(kinds),
                                            _lib.buf(sigs) if signer else None, _lib.buf(voted) if signer else None))
    return codes, dig, kinds, sigs, voted


VOTE_BATCH = ["hdr-ok", "vote-ok", "hdr-bad-sig", "cert-ok", "hdr-bad-id", "request", "hdr-too-old", "truncated",
              "hdr-long-key", "empty", "hdr-no-stake", "vote-stale-target", "cert-bad-vote", "hdr-ok-last"]


def vote_batch(f):
    """The headers whose votes are checked, among non-headers; an Ok header last, so that the
    bounded read of its round ends at the batch's last bytes."""
    return [f[n] for n in VOTE_BATCH]


def dev_ex(lib, items, signer, stream, own_state=True):
    """nwc_dev_sanitize_messages_ex over torch tensors on `stream` -> (rc, outputs as run_ex's)."""
    import torch
    data, offs, gcs, tg = pack(items)
    m = len(items)
    total = int(offs[-1])
    with torch.cuda.stream(stream):
        d_data = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        d_data[:total] = torch.from_numpy(data[:total]).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        d_gcs = torch.from_numpy(gcs.astype(np.int64)).cuda()
        d_tg = torch.from_numpy(tg).cuda()
        d_codes = torch.full((m,), -99, dtype=torch.int32, device="cuda")
        d_dig = torch.full((m, 32), 0xEE, dtype=torch.uint8, device="cuda")
        d_kinds = torch.full((m,), 0xEE, dtype=torch.uint8, device="cuda")
        d_sigs = torch.full((m, 64), 0xEE, dtype=torch.uint8, device="cuda")
        d_voted = torch.full((m,), 0xEE, dtype=torch.uint8, device="cuda")
    stream.synchronize()
    rc = lib.nwc_dev_sanitize_messages_ex(d_data.data_ptr(), d_offs.data_ptr(), m, total,
                                          d_gcs.data_ptr() if own_state else None, 0,
                                          d_tg.data_ptr() if own_state else None, None, signer, d_codes.data_ptr(),
                                          d_dig.data_ptr(), d_kinds.data_ptr(), d_sigs.data_ptr() if signer else None,
                                          d_voted.data_ptr() if signer else None, stream.cuda_stream)
    stream.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (d_codes, d_dig, d_kinds, d_sigs, d_voted))


def message_cuts(hoff, m, msg_chunk):
    """msg_plan.h message_cuts, restated."""
    total, cuts, lo = int(hoff[m]), [0], min(8 << 20, msg_chunk)
    hl = [int(x) for x in hoff]
    if total >= (4 << 20) and msg_chunk and total >= 4 * lo:
        at, nxt = 0, min(msg_chunk, 2 * lo)
        while total - at > 2 * lo:
            want = max(lo, min(nxt, (total - at) // 2))
            cm = bisect.bisect_left(hl, at + want) & ~63
            if cm <= cuts[-1]:
                cm = cuts[-1] + 64
            if cm >= m:
                break
            cuts.append(cm)
            at, nxt = hl[cm], min(msg_chunk, 2 * nxt)
    cuts.append(m)
    return cuts


def _make_signer(lib, w):
    from narwhal_amd import _lib
    seed = w.seeds[SIGNER_KEY]
    h = lib.nwc_signer_create(_lib.buf(seed + w.pks[SIGNER_KEY]))
    assert h, lib.nwc_last_error()
    return h


def _chunked(lib, w):
    chunk = int(os.environ["NWC_MSG_CHUNK"])
    f = fixture(w)
    names = ["hdr-ok", "vote-ok", "cert-ok", "hdr-long-key", "truncated", "hdr-at-gc", "vote-no-target", "request",
             "hdr-bad-sig", "cert-bad-vote", "hdr-ok-last", "empty", "hdr-no-stake"]
    tile = [f[n] for n in names]
    per = sum(len(t[0]) for t in tile)
    reps = (4 << 20) // per + 1
    items = [tile[i % len(tile)] for i in range(reps * len(tile))]
    hoff = np.zeros(len(items) + 1, np.uint64)
    hoff[1:] = np.cumsum([len(it[0]) for it in items])
    m, total = len(items), int(hoff[-1])
    cuts = message_cuts(hoff, m, chunk)
    # the first and last message of every chunk: a stale state (headers and certificates TooOld,
    # votes UnexpectedVote), unlike their neighbours'
    stale = (w.rand32(), 7, w.pks[1])
    edges = sorted(set(cuts[:-1]) | set(c - 1 for c in cuts[1:]))
    eset = set(edges)
    for i in edges:
        items[i] = (items[i][0], STALE_GC, stale)
    signer = _make_signer(lib, w)
    first = run_ex(lib, items, signer)
    second = run_ex(lib, items, signer)   # twice on the same stages and arena
    # the same batch in calls of at most 1 MiB (each takes the single copy)
    parts, lo = [], 0
    while lo < m:
        hi = lo + 1
        while hi < m and int(hoff[hi + 1]) - int(hoff[lo]) <= (1 << 20):
            hi += 1
        parts.append(run_ex(lib, items[lo:hi], signer))
        lo = hi
    ref = [np.concatenate([p[k] for p in parts]) for k in range(5)]
    plain = run_ex(lib, items, None)
    codes = first[0]
    out = {"m": m, "total": total, "cuts": cuts, "calls": len(parts),
           "same": [bool((a == b).all()) for a, b in zip(first, ref)],
           "same_twice": [bool((a == b).all()) for a, b in zip(first, second)],
           "same_without_signer": [bool((a == b).all()) for a, b in zip(first[:3], plain[:3])],
           "edge_codes_differ": int(sum(1 for i in edges if codes[i] != EXPECTED_CODES[names[i % len(names)]])),
           "edges": len(edges),
           "neighbours_unchanged": bool(all(codes[i] == EXPECTED_CODES[names[i % len(names)]] for i in range(m) if i not in eset)),
           "voted_per_chunk": [int(first[4][cuts[k]:cuts[k + 1]].sum()) for k in range(len(cuts) - 1)],
           "voted_is_ok_header": bool(((first[4] == 1) == ((codes == 0) & (first[2] == 0))).all()),
           "unvoted_sigs_zero": bool((first[3][first[4] == 0] == 0).all()),
           "destroy": lib.nwc_signer_destroy(signer)}
    return out


def _wrong_device(lib, w):
    import torch
    from narwhal_amd import _lib
    out = {"devices": lib.nwc_device_count()}
    _lib.check(lib.nwc_dev_set_device(1))
    signer1 = _make_signer(lib, w)
    _lib.check(lib.nwc_dev_set_device(0))
    signer0 = _make_signer(lib, w)
    f = fixture(w)
    items = vote_batch(f)
    rc, got = dev_ex(lib, items, signer1, torch.cuda.Stream())
    out["dev_rc"], out["dev_code"] = rc, lib.nwc_last_error_code()
    out["dev_votes_zero"] = bool((got[3] == 0).all() and (got[4] == 0).all())
    rc0, got0 = dev_ex(lib, items, signer0, torch.cuda.Stream())
    host1 = run_ex(lib, items, signer1)    # runs whole on context 1
    host0 = run_ex(lib, items, signer0)
    out["dev_rc_same_device"] = rc0
    out["host_matches"] = [bool((a == b).all()) for a, b in zip(host1, host0)]
    out["dev_matches"] = [bool((a == b).all()) for a, b in zip(got0, host0)]
    out["voted"] = [int(x) for x in host1[4]]
    out["codes"] = [int(x) for x in host1[0]]
    out["sigs"] = bytes(host1[3]).hex()
    # without a signer a call of >= 4,096 messages is sharded over the two contexts: each range
    # takes its own slice of the per-message arrays
    big = [f[VOTE_BATCH[i % len(VOTE_BATCH)]] for i in range(300 * len(VOTE_BATCH))]
    codes, _, kinds, _, _ = run_ex(lib, big, None)
    out["sharded_m"] = len(big)
    out["sharded_codes_ok"] = bool(all(int(codes[i]) == EXPECTED_CODES[VOTE_BATCH[i % len(VOTE_BATCH)]] for i in range(len(big))))
    out["sharded_kinds_ok"] = bool(all(int(kinds[i]) == int(kinds[i % len(VOTE_BATCH)]) for i in range(len(big))))
    out["destroy"] = [lib.nwc_signer_destroy(signer0), lib.nwc_signer_destroy(signer1)]
    return out


def _sign_table_address(lib):
    addr, n = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.nwc_diag_table(b"sign_table", ctypes.byref(addr), None, ctypes.byref(n), None) == 0
    return int(addr.value)


def _memory(lib, w):
    from narwhal_amd import _lib
    f = fixture(w)
    items = [f[n] for n in ("hdr-ok", "vote-ok", "cert-ok", "hdr-too-old", "empty")]
    out = {"tables_start": _lib.memory_info()["tables"], "sign_table_start": _sign_table_address(lib)}
    got = run_ex(lib, items, None)
    plain = run_ex(lib, items, None, own_state=False)
    out["codes"] = [int(c) for c in got[0]]
    out["codes_plain"] = [int(c) for c in plain[0]]
    out["tables_after_ex"] = _lib.memory_info()["tables"]
    out["sign_table_after_ex"] = _sign_table_address(lib)
    signer = _make_signer(lib, w)
    out["sign_table_with_signer"] = _sign_table_address(lib) != 0
    out["tables_with_signer"] = _lib.memory_info()["tables"]
    voted = run_ex(lib, items, signer)[4]
    out["voted"] = [int(v) for v in voted]
    out["destroy"] = lib.nwc_signer_destroy(signer)
    return out


if __name__ == "__main__":
    from narwhal_amd import _lib  # noqa: E402
    from tests.oracle_lib import load_oracle  # noqa: E402
    lib_ = _lib.load()
    w_ = ExWorld(load_oracle())
    w_.install(lib_)
    print(json.dumps({"chunked": _chunked, "wrong_device": _wrong_device, "memory": _memory}[sys.argv[1]](lib_, w_)))
