"""Callers and child processes of tests/test_gpu_sanitizer_view.py (nwc_sanitizer_sanitize_view,
nwc_sanitizer_view_stats).

Imported, it gives the ctypes caller of the handle's view entry and the check of one answer against
the model (tests/msg_view_model.py) and against nwc_sanitize_messages_view on the same message
alone.  Run as a program it is a child process, because libnwc reads its environment once per
process and nwc_shutdown ends a process's use of the device:

  bypass    NWC_SANITIZER_GROUP_BYTES=4096 in the environment: a certificate longer than 8 KiB goes
            round the groups and returns its exact view; then, while the cache is not the configured
            committee, the call answers as nwc_sanitize_messages_view does
  scratch   a fresh process: the HBM scratch a sanitizer holds at create, and after view requests
  shutdown  nwc_shutdown with a live sanitizer and four viewers blocked in a group

usage: sanitizer_view_helper.py MODE ROOT; prints one JSON line."""
import ctypes
import json
import os
import struct
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[2])
    sys.path.insert(0, os.path.join(sys.argv[2], "oracle"))

from tests.msg_view_helper import Model, check_views, run_view  # noqa: E402
from tests.test_gpu_sanitizer import LONG_WAIT_US, NOT_INIT, S, _World  # noqa: E402

ERR_ARG = -2


class Answer:
    """What one nwc_sanitizer_sanitize_view call left: every output starts as 0xEE (voted as 7)."""

    def __init__(self, rc, dig, kind, sig, voted, rec, body, used):
        self.rc, self.dig, self.kind, self.sig, self.voted, self.rec, self.body, self.used = rc, dig, kind, sig, voted, rec, body, used

    def plain(self):
        return self.rc, self.dig, self.kind


class SW(S):
    """A sanitizer handle with the view entry."""

    def view(self, msg, gc_round=0, target=None, signer=None, view=True, cap=None):
        from narwhal_amd import _lib
        tb = None if target is None else target[0] + struct.pack("<Q", target[1]) + target[2]
        dig, kind = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
        sig = ctypes.create_string_buffer(b"\xEE" * 64, 64)
        voted = ctypes.c_int32(7)
        rec = np.full(160, 0xEE, np.uint8)
        bound = int(self.lib.nwc_msg_view_body_bound(len(msg), 1))
        cap = bound if cap is None else cap
        body = np.full(bound, 0xEE, np.uint8)
        used = ctypes.c_uint64(0xEEEE)
        rc = self.lib.nwc_sanitizer_sanitize_view(self.h, signer, _lib.buf(msg) if msg else None, len(msg), gc_round,
                                                  _lib.buf(tb) if tb else None, dig, kind, sig, ctypes.byref(voted),
                                                  _lib.buf(rec) if view else None, _lib.buf(body), cap, ctypes.byref(used))
        return Answer(rc, dig.raw, kind.raw[0], sig.raw, voted.value, rec, body, int(used.value))

    def view_stats(self):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert self.lib.nwc_sanitizer_view_stats(self.h, ctypes.byref(a), ctypes.byref(b)) == 0
        return {"in_flight": int(a.value), "alone": int(b.value)}

    def group(self, jobs):
        """The jobs -- (msg, gc_round, target, ask for a view, signer or None) -- in ONE group of this
        sanitizer, job k in slot k: each is started once the previous one has joined."""
        base = self.stats()["messages"]
        with ThreadPoolExecutor(len(jobs)) as pool:
            futs = []
            for k, (msg, gc, target, ask, signer) in enumerate(jobs):
                futs.append(pool.submit(self.view, msg, gc, target, signer, ask))
                self.wait_messages(base + k + 1)
            return [f.result(timeout=60) for f in futs]


def alone(lib, item, signer=None):
    """nwc_sanitize_messages_view on the one message: run_view's outputs."""
    return run_view(lib, [item], signer)


def check_answer(lib, model, item, a, what, signer=None, ref=None):
    """One answer that asked for a view: all 160 bytes of the record, body_used and the body areas the
    record names against nwc_sanitize_messages_view on the message alone (ref: that call's outputs, if
    the caller made it already), and field for field against the model.  The model is the independent
    reference: the batch entry's kernel shares its body (message_view) with k_view_group, so the
    byte comparison shows that the two routes agree, not that the shared body is right.  Returns the
    alone call."""
    ref = alone(lib, item, signer) if ref is None else ref
    codes, dig, kinds, sigs, voted, recs, body, used = ref
    assert a.rc == int(codes[0]), (what, a.rc, int(codes[0]))
    assert a.kind == int(kinds[0]), what
    if a.kind != 3:
        assert a.dig == dig[0].tobytes(), what
    assert a.rec.tobytes() == recs[0].tobytes(), (what, a.rec.tobytes().hex(), recs[0].tobytes().hex())
    assert a.used == used, (what, a.used, used)
    # the body areas the record names, byte for byte (the padding that rounds an area up to 16 bytes
    # is nobody's: the batch entry returns whatever its arena held there)
    flags, (n_pay, n_par, n_votes), (p_off, q_off, v_off) = int(a.rec[2]), struct.unpack_from("<III", a.rec, 120), \
        struct.unpack_from("<QQQ", a.rec, 136)
    areas = ([(p_off, 36 * n_pay)] if flags & 1 else []) + ([(q_off, 32 * n_par)] if flags & 2 else []) + [(v_off, 8 * n_votes)]
    for at, n in areas:
        assert at + n <= used, (what, at, n, used)
        assert a.body[at:at + n].tobytes() == body[at:at + n].tobytes(), (what, at, n)
    assert (a.body[used:] == 0xEE).all(), what          # only body_used bytes came back
    if signer:
        assert a.voted == int(voted[0]) and a.sig == (sigs[0].tobytes() if voted[0] else bytes(64)), what
    else:
        assert a.voted == 7 and a.sig == b"\xEE" * 64, what   # without a signer the vote outputs are ignored
    got = (np.array([a.rc], np.int32), None, None, None, None, a.rec.reshape(1, 160), a.body, a.used)
    check_views([item], got, model, what)
    return ref


def _main():
    from narwhal_amd import _lib
    from tests.oracle_lib import load_oracle
    mode = sys.argv[1]
    lib = _lib.load()
    w = _World(load_oracle(), 66, 7)
    w.install(lib)
    model = Model(w.pks)
    out = {}
    if mode == "bypass":
        cert = w.certificate(2, 6, list(range(66)), nparents=66)
        vote = w.vote(3, w.rand32(), 4, w.pks[5])
        with SW(lib, 0, 0) as s:
            a = s.view(cert)
            check_answer(lib, model, (cert, 0, None), a, "bypassed certificate")
            exp = w.expect(cert)
            out["cert_len"] = len(cert)
            out["cert_ok"] = a.rc == exp[0] == 0 and a.dig == exp[2] and a.kind == 2
            out["after_cert"] = dict(s.stats(), **s.view_stats())
            a = s.view(vote)
            check_answer(lib, model, (vote, 0, None), a, "grouped vote")
            out["after_vote"] = dict(s.stats(), **s.view_stats())
            # the cache is not the configured committee: the call answers as the batch entry does
            other = _World(w.o, 4, 99)
            _lib.check(lib.nwc_set_committee(_lib.buf(b"".join(other.pks)), 4))
            offs = np.array([0, len(vote)], np.uint64)
            codes = np.zeros(1, np.int32)
            rec = np.full(160, 0xEE, np.uint8)
            body = np.zeros(len(vote) + 64, np.uint8)
            used = ctypes.c_uint64(5)
            parent = lib.nwc_sanitize_messages_view(_lib.buf(vote), _lib.buf(offs), 1, None, 0, None, None, None, _lib.buf(codes),
                                                    None, None, None, None, _lib.buf(rec), _lib.buf(body), len(body),
                                                    ctypes.byref(used))
            a = s.view(vote)
            out["unconfigured"] = {"parent": parent, "rc": a.rc, "record_zero": bool((a.rec == 0).all()), "used": a.used,
                                   "parent_record_zero": bool((rec == 0).all()), "parent_used": int(used.value)}
            out["after_unconfigured"] = dict(s.stats(), **s.view_stats())
            w.install(lib)
            a = s.view(vote)
            check_answer(lib, model, (vote, 0, None), a, "configured again")
            out["after_configured"] = dict(s.stats(), **s.view_stats())
    elif mode == "scratch":
        hdr = w.mr.msg_header(w.header(1, 3, 5)[0])
        run_view(lib, [(hdr, 0, None)])   # (the batch entry's own buffers are allocated before the walk)
        _lib.check(lib.nwc_trim())
        mem0 = _lib.memory_info()["scratch"]
        with SW(lib, 0, 0) as s:
            out["at_create"] = _lib.memory_info()["scratch"] - mem0
            plain = s.raw(hdr)
            a = s.view(hdr, view=False)
            out["null_view_same"] = a.plain() == plain and a.used == 0xEEEE and bool((a.body == 0xEE).all())
            _lib.check(lib.nwc_trim())   # (what the launches' own paths grew on demand goes; a sanitizer's scratch stays)
            out["never_viewed"] = _lib.memory_info()["scratch"] - mem0
            a = s.view(hdr)
            check_answer(lib, model, (hdr, 0, None), a, "header")
            _lib.check(lib.nwc_trim())
            out["after_views"] = _lib.memory_info()["scratch"] - mem0
            out["view_stats"] = s.view_stats()
    elif mode == "shutdown":
        msgs = [w.mr.msg_header(w.header(1, 3, 5)[0]), w.vote(3, w.rand32(), 4, w.pks[5]), w.certificate(2, 6, list(range(45))),
                b"\x02\x00\x00\x00\x07"]
        refs = [alone(lib, (b, 0, None)) for b in msgs]
        s = SW(lib, 8, LONG_WAIT_US)   # the group waits for company: the four viewers block in it
        with ThreadPoolExecutor(4) as pool:
            futs = [pool.submit(s.view, b) for b in msgs]
            s.wait_messages(4)
            lib.nwc_shutdown()
            got = [f.result(timeout=60) for f in futs]
        out["rcs"] = [a.rc for a in got]
        right = 0
        for k, (a, b) in enumerate(zip(got, msgs)):
            if a.rc == NOT_INIT:
                assert (a.rec == 0).all() and a.used == 0, k
                continue
            assert a.rc >= 0, (k, a.rc)
            # (the library is shut down: the reference call was made before)
            check_answer(lib, model, (b, 0, None), a, "shutdown %d" % k, ref=refs[k])
            right += 1
        out["right"] = right
        a = s.view(msgs[0])
        out["after_shutdown"] = [a.rc, bool((a.rec == 0).all()), a.used]
        out["destroy"] = lib.nwc_sanitizer_destroy(s.h)
        s.h = None
    print(json.dumps(out))


if __name__ == "__main__":
    _main()
