"""Callers and child processes of tests/test_gpu_msg_view.py (nwc_sanitize_messages_view,
nwc_dev_sanitize_messages_view).

Imported, it gives the ctypes callers and the check of one call against the model
(tests/msg_view_model.py) and against nwc_sanitize_messages_ex.  Run as a program it is a child
process, because libnwc reads its environment once per process:

  chunked      NWC_MSG_CHUNK=1048576 in the environment: the fixture messages of
               tests/sanitize_ex_helper.py tiled to just over 4 MiB, so the call is staged and cut;
               every view against the model, the messages around the cuts included
  scratch_ex   one nwc_sanitize_messages_ex call, then nwc_memory_info().scratch
  scratch_view the same call through nwc_sanitize_messages_view with views == NULL

usage: msg_view_helper.py MODE ROOT; prints one JSON line."""
import ctypes
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[2])
    sys.path.insert(0, os.path.join(sys.argv[2], "oracle"))

from tests import msg_view_model as vm  # noqa: E402
from tests.sanitize_ex_helper import ExWorld, fixture, message_cuts, pack, run_ex  # noqa: E402


def run_view(lib, items, signer=None, own_state=True, views=True, digests=True):
    """nwc_sanitize_messages_view over the items -> (codes, digests, kinds, vote_sigs, voted, records
    (m x 160), body, body_used); every output starts as 0xEE, as run_ex's."""
    from narwhal_amd import _lib
    data, offs, gcs, tg = pack(items)
    m = len(items)
    codes = np.full(m, -99, np.int32)
    dig = np.full((m, 32), 0xEE, np.uint8)
    kinds = np.full(m, 0xEE, np.uint8)
    sigs = np.full((m, 64), 0xEE, np.uint8)
    voted = np.full(m, 0xEE, np.uint8)
    recs = np.full((m, 160), 0xEE, np.uint8)
    cap = int(lib.nwc_msg_view_body_bound(int(offs[-1]), m))
    body = np.full(cap, 0xEE, np.uint8)
    used = ctypes.c_uint64(0xEEEE)
    _lib.check(lib.nwc_sanitize_messages_view(_lib.buf(data), _lib.buf(offs), m, _lib.buf(gcs) if own_state else None, 0,
                                              _lib.buf(tg) if own_state else None, None, signer,
                                              _lib.buf(codes), _lib.buf(dig) if digests else None, _lib.buf(kinds),
                                              _lib.buf(sigs) if signer else None, _lib.buf(voted) if signer else None,
                                              _lib.buf(recs) if views else None, _lib.buf(body) if views else None,
                                              cap if views else 0, ctypes.byref(used) if views else None))
    return codes, dig, kinds, sigs, voted, recs, body, int(used.value)


class Model:
    """The expected view of each distinct (message, code), computed once."""

    def __init__(self, keys):
        self.keys, self.memo = list(keys), {}

    def of(self, msg, code):
        if (msg, code) not in self.memo:
            self.memo[(msg, code)] = vm.expected(msg, self.keys, code)
        return self.memo[(msg, code)]


def check_views(items, got, model, what=""):
    """The records, the body and body_used of one call against the model; returns the records."""
    codes, recs, body, used = got[0], got[5], got[6], got[7]
    m = len(items)
    total = sum(len(it[0]) for it in items)
    assert used % 16 == 0 and used <= vm.body_bound(total, m), (what, used)
    assert (body[used:] == 0xEE).all(), what            # only body_used bytes came back
    out = []
    bb = body.tobytes()
    for i, it in enumerate(items):
        rec = recs[i].tobytes()
        out.append(vm.check_against(rec, bb, used, model.of(it[0], int(codes[i])), it[0], (what, i)))
    vm.check_disjoint(out, used)
    return out


def view_and_ex(lib, items, model, signer=None, what=""):
    """One view call against the same _ex call (byte-identical outputs) and against the model."""
    ex = run_ex(lib, items, signer)
    got = run_view(lib, items, signer)
    for k, (a, b) in enumerate(zip(ex, got[:5])):
        assert a.tobytes() == b.tobytes(), (what, "output", k)
    return got, check_views(items, got, model, what)


def dev_view(lib, items, signer, stream):
    """nwc_dev_sanitize_messages_view over torch tensors on `stream` -> (rc, run_view's outputs);
    d_body_used is read after the stream has been synchronised."""
    import torch
    data, offs, gcs, tg = pack(items)
    m = len(items)
    total = int(offs[-1])
    cap = int(lib.nwc_msg_view_body_bound(total, m))
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
        d_recs = torch.full((m, 160), 0xEE, dtype=torch.uint8, device="cuda")
        d_body = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
        d_used = torch.full((1,), 0x7777, dtype=torch.int64, device="cuda")
    stream.synchronize()
    rc = lib.nwc_dev_sanitize_messages_view(d_data.data_ptr(), d_offs.data_ptr(), m, total, d_gcs.data_ptr(), 0,
                                            d_tg.data_ptr(), None, signer, d_codes.data_ptr(), d_dig.data_ptr(),
                                            d_kinds.data_ptr(), d_sigs.data_ptr() if signer else None,
                                            d_voted.data_ptr() if signer else None, d_recs.data_ptr(), d_body.data_ptr(), cap,
                                            d_used.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    used = int(d_used.cpu().numpy()[0])
    body = d_body.cpu().numpy()
    host_body = np.full(cap, 0xEE, np.uint8)
    host_body[:used] = body[:used]
    assert (body[used:] == 0xEE).all()   # nothing is written past the allocator's final value
    return rc, tuple(t.cpu().numpy() for t in (d_codes, d_dig, d_kinds, d_sigs, d_voted, d_recs)) + (host_body, used)


def _chunked(lib, w):
    chunk = int(os.environ["NWC_MSG_CHUNK"])
    f = fixture(w)
    # unsorted parents in every tile: body areas in every chunk, among fast- and slow-path certificates
    hid = w.rand32()
    unsorted = w.mr.msg_header(w.mr.enc_header(w.pks[0], 5, [], [b"\x09" * 32, b"\x03" * 32, b"\x09" * 32], hid, bytes(64),
                                               wire_order=True))
    names = ["hdr-ok", "vote-ok", "cert-ok", "hdr-long-key", "truncated", "hdr-at-gc", "vote-no-target", "request",
             "hdr-bad-sig", "cert-bad-vote", "hdr-ok-last", "empty", "hdr-no-stake"]
    tile = [f[n] for n in names] + [(unsorted, 0, None), (w.certificate(1, 3, [0, 1, 2], unpadded_vote=1), 0, None)]
    per = sum(len(t[0]) for t in tile)
    reps = (4 << 20) // per + 1
    items = [tile[i % len(tile)] for i in range(reps * len(tile))]
    hoff = np.zeros(len(items) + 1, np.uint64)
    hoff[1:] = np.cumsum([len(it[0]) for it in items])
    m, total = len(items), int(hoff[-1])
    cuts = message_cuts(hoff, m, chunk)
    model = Model(w.pks)
    ex = run_ex(lib, items)
    got = run_view(lib, items)
    recs = check_views(items, got, model, "chunked")
    around = sorted(set(i for c in cuts[1:-1] for i in (c - 1, c, c + 1) if 0 <= i < m))
    return {"m": m, "total": total, "cuts": cuts, "same_as_ex": [a.tobytes() == b.tobytes() for a, b in zip(ex[:3], got[:3])],
            "checked": len(recs), "around_cuts": len(around), "decoded_around_cuts": int(sum(recs[i]["decoded"] for i in around)),
            "decoded": int(sum(r["decoded"] for r in recs)), "in_body": int(sum(1 for r in recs if r["flags"])),
            "voters": int(sum(r["n_votes"] for r in recs)), "body_used": got[7],
            "d2h_bytes_per_message": (160 * m + got[7]) / m}


def _scratch(lib, w, through_view):
    from narwhal_amd import _lib
    f = fixture(w)
    items = [f[n] for n in ("hdr-ok", "vote-ok", "cert-ok", "hdr-too-old", "empty")]
    got = run_view(lib, items, views=False) if through_view else run_ex(lib, items)
    return {"codes": [int(c) for c in got[0]], "digests": got[1].tobytes().hex(), "kinds": [int(k) for k in got[2]],
            "scratch": _lib.memory_info()["scratch"]}


if __name__ == "__main__":
    from narwhal_amd import _lib  # noqa: E402
    from tests.oracle_lib import load_oracle  # noqa: E402
    lib_ = _lib.load()
    w_ = ExWorld(load_oracle())
    w_.install(lib_)
    mode = sys.argv[1]
    if mode == "chunked":
        print(json.dumps(_chunked(lib_, w_)))
    else:
        print(json.dumps(_scratch(lib_, w_, mode == "scratch_view")))
