"""nwc_sanitize_messages_view without a device (include/nwc.h): the model of the view record
(tests/msg_view_model.py) against the golden wire fixtures and against hand-built messages with
unsorted and duplicated entries; the three new exports; the ctypes record against the header's
layout; and the argument conventions, which answer before anything touches a GPU, in a fresh
process that never calls nwc_init."""
import ctypes
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np

from tests import msg_view_model as vm
from tests.conftest import GOLDEN, ROOT

mr = vm.mr
LIB = os.path.join(ROOT, "narwhal_amd", "libnwc.so")
HEADER = os.path.join(ROOT, "include", "nwc.h")


def _golden():
    g = json.load(open(os.path.join(GOLDEN, "messages.json")))
    return [bytes.fromhex(k) for k in g["committee"]["keys"]], g["cases"]


def _roundtrip(msgs, keys, codes):
    """model -> records + body -> rebuilt objects, each against mr.decode of its wire"""
    views = [vm.expected(m, keys, c) for m, c in zip(msgs, codes)]
    recs, body = vm.pack(views)
    assert len(recs) == 160 * len(msgs)
    assert len(body) <= vm.body_bound(sum(len(m) for m in msgs), len(msgs))
    got = [vm.unpack(recs[160 * i:160 * i + 160]) for i in range(len(msgs))]
    vm.check_disjoint(got, len(body))
    for i, m in enumerate(msgs):
        kind, f = mr.decode(m)
        rk, rf = vm.rebuild(recs[160 * i:160 * i + 160], m, body, keys)
        if kind in (0, 1, 2):
            assert (rk, rf) == (kind, f), i
            vm.check_against(recs[160 * i:160 * i + 160], body, len(body), views[i], m, i)
        else:
            assert rk is None and got[i]["decoded"] == 0, i
            assert recs[160 * i + 8:160 * i + 160] == bytes(152), i
    return got


def test_model_on_every_golden_fixture():
    keys, cases = _golden()
    msgs = [bytes.fromhex(c["msg"]) for c in cases]
    got = _roundtrip(msgs, keys, [c["code"] for c in cases])
    for c, v in zip(cases, got):
        # decoded: every code except SerializationError, UnexpectedMessage and DecodePanic
        assert v["decoded"] == (0 if c["code"] in (8, 10, 11) else 1), c["name"]
        assert v["code"] == c["code"], c["name"]
        if c["kind"] >= 0:
            assert v["kind"] == c["kind"], c["name"]
    by = {c["name"]: v for c, v in zip(cases, got)}
    assert by["ref-header"]["flags"] == 0 and by["header-many-parents"]["flags"] == 0
    assert by["header-unsorted-parents"]["flags"] == vm.PARENTS_IN_BODY
    assert by["header-unsorted-payload"]["flags"] == vm.PAYLOAD_IN_BODY
    assert by["header-duplicate-payload-same"]["flags"] & vm.PAYLOAD_IN_BODY
    assert by["header-many-unsorted"]["flags"] & vm.PARENTS_IN_BODY


def _hdr(rng, payload, parents, wire_order=True, cert_votes=None):
    author = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    hid = mr.header_id(author, 9, payload, parents)
    h = mr.enc_header(author, 9, payload, parents, hid, bytes(64), wire_order=wire_order)
    if cert_votes is None:
        return mr.msg_header(h)
    return mr.msg_certificate(h, cert_votes)


def test_model_on_unsorted_and_duplicate_entries():
    rng = np.random.default_rng(3)
    r32 = lambda: bytes(rng.integers(0, 256, 32, dtype=np.uint8))  # noqa: E731
    keys = [r32() for _ in range(4)]
    d = sorted(r32() for _ in range(5))
    votes = [(keys[2], bytes(64)), (r32(), bytes(64)), (keys[0], bytes(64))]
    msgs = [
        _hdr(rng, [(d[2], 1), (d[0], 2), (d[2], 7)], [d[1], d[0]]),            # duplicate key: the LAST value stays
        _hdr(rng, [(d[0], 1), (d[1], 2)], [d[3], d[3], d[1]]),                   # payload ascending, parents not
        _hdr(rng, [(d[1], 1), (d[0], 2)], [d[1], d[3]]),                         # the reverse
        _hdr(rng, [(d[0], 1), (d[0], 2)], []),                                   # equal neighbours are not ascending
        _hdr(rng, [(d[4], 3), (d[3], 2), (d[4], 1)], [d[2], d[1], d[2]], cert_votes=votes),
        _hdr(rng, [], [], cert_votes=[]),
    ]
    got = _roundtrip(msgs, keys, [0] * len(msgs))
    assert [v["flags"] for v in got] == [3, 2, 1, 1, 3, 0]
    assert (got[0]["n_payload"], got[0]["n_parents"]) == (2, 2)
    first = vm.expected(msgs[0], keys, 0)
    assert first["payload"] == [(d[0], 2), (d[2], 7)]
    assert (got[3]["n_payload"], got[4]["n_payload"], got[4]["n_parents"], got[4]["n_votes"]) == (1, 2, 2, 3)
    assert [k for k, _ in vm.expected(msgs[4], keys, 0)["votes"]] == [2, -1, 0]
    assert got[5]["n_votes"] == 0 and got[5]["votes_off"] == 0


def test_library_exports_the_three_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert {"nwc_sanitize_messages_view", "nwc_dev_sanitize_messages_view", "nwc_msg_view_body_bound"} <= exported


def _header_layout():
    """field -> (offset, size) of nwc_msg_view, computed from the struct's text in include/nwc.h"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nwc_msg_view \{(.*?)\} nwc_msg_view;", text, flags=re.S).group(1)
    size = {"uint8_t": 1, "int32_t": 4, "uint32_t": 4, "uint64_t": 8}
    out, at = {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s+(\w+)(?:\[(\d+)\])?$", decl)
        assert m, decl
        n = size[m.group(1)]
        at = (at + n - 1) // n * n   # natural alignment
        total = n * int(m.group(3) or 1)
        out[m.group(2)] = (at, total)
        at += total
    return out, (at + 7) // 8 * 8


def test_ctypes_record_matches_the_header():
    from narwhal_amd import _lib
    layout, total = _header_layout()
    assert total == 160 and ctypes.sizeof(_lib.MsgView) == 160
    assert [n for n, _ in _lib.MsgView._fields_] == list(layout) == list(vm.FIELDS)
    for name, (at, n) in layout.items():
        f = getattr(_lib.MsgView, name)
        assert (f.offset, f.size) == (at, n) and vm.OFFSETS[name] == at, name
    assert (_lib.VIEW_PAYLOAD_IN_BODY, _lib.VIEW_PARENTS_IN_BODY) == (1, 2)
    text = open(HEADER).read()
    assert "#define NWC_VIEW_PAYLOAD_IN_BODY 1" in text and "#define NWC_VIEW_PARENTS_IN_BODY 2" in text


CHILD = r'''
import ctypes, json, sys
sys.path.insert(0, %r)
from narwhal_amd import _lib
lib = _lib.load(init=False)
out = {}
data = bytes(1000)
offs = (ctypes.c_uint64 * 4)(0, 300, 700, 1000)
m = 3
bound = lib.nwc_msg_view_body_bound(1000, 3)
out["bound"] = bound
out["bound_big"] = lib.nwc_msg_view_body_bound(1 << 40, 1 << 33)
codes = (ctypes.c_int32 * 3)(77, 77, 77)
p = _lib.buf(data)
def fresh():
    return ctypes.create_string_buffer(b"\xff" * 480, 480), ctypes.create_string_buffer(b"\xff" * bound, bound), ctypes.c_uint64(99)
def call(views, body, cap, used, n=m, signer=None, sigs=None, voted=None):
    return lib.nwc_sanitize_messages_view(p, offs, n, None, 0, None, None, signer, codes, None, None, sigs, voted,
                                          views, body, cap, ctypes.byref(used) if used is not None else None)
v, b, u = fresh()
out["null_body"] = call(v, None, bound, u)
out["null_body_code"] = lib.nwc_last_error_code()
out["null_body_zeroed"] = v.raw == bytes(480) and u.value == 0
v, b, u = fresh()
out["null_used"] = call(v, b, bound, None)
v, b, u = fresh()
out["cap_below"] = call(v, b, bound - 1, u)
out["cap_below_zeroed"] = v.raw == bytes(480) and u.value == 0
v, b, u = fresh()
out["m0"] = call(v, b, 0, u, n=0)
out["m0_untouched"] = v.raw == b"\xff" * 480 and b.raw == b"\xff" * bound and u.value == 99
v, b, u = fresh()
out["not_init"] = call(v, b, bound, u)
out["not_init_code"] = lib.nwc_last_error_code()
out["not_init_text"] = lib.nwc_last_error().decode()
out["not_init_zeroed"] = v.raw == bytes(480) and u.value == 0
out["body_untouched"] = b.raw == b"\xff" * bound
# views == NULL: the entry is nwc_sanitize_messages_ex, body arguments ignored
out["no_views"] = lib.nwc_sanitize_messages_view(p, offs, m, None, 0, None, None, None, codes, None, None, None, None,
                                                 None, None, 0, None)
out["no_views_ex"] = lib.nwc_sanitize_messages_ex(p, offs, m, None, 0, None, None, None, codes, None, None, None, None)
# a signer with NULL vote outputs, as nwc_sanitize_messages_ex (the signer is not dereferenced for that)
fake = ctypes.c_void_p(0x1000)
v, b, u = fresh()
out["signer_null_outputs"] = call(v, b, bound, u, signer=fake)
# the device entry
out["dev_null_body"] = lib.nwc_dev_sanitize_messages_view(p, p, 3, 1000, None, 0, None, None, None, p, None, None, None, None,
                                                          p, None, bound, p, None)
out["dev_cap_below"] = lib.nwc_dev_sanitize_messages_view(p, p, 3, 1000, None, 0, None, None, None, p, None, None, None, None,
                                                          0x1000, 0x2000, bound - 1, 0x3000, None)
out["dev_m0"] = lib.nwc_dev_sanitize_messages_view(None, None, 0, 0, None, 0, None, None, None, None, None, None, None, None,
                                                   0x1000, None, 0, None, None)
out["dev_not_init"] = lib.nwc_dev_sanitize_messages_view(p, p, 3, 1000, None, 0, None, None, None, p, None, None, None, None,
                                                         0x1000, 0x2000, bound, 0x3000, None)
out["dev_no_views"] = lib.nwc_dev_sanitize_messages_view(p, p, 3, 1000, None, 0, None, None, None, p, None, None, None, None,
                                                         None, None, 0, None, None)
out["codes_untouched"] = list(codes) == [77, 77, 77]
# a message of 2^32 bytes (only its offsets are read before the refusal)
big = (ctypes.c_uint64 * 2)(0, 1 << 32)
v, b, u = fresh()
out["too_long"] = lib.nwc_sanitize_messages_view(p, big, 1, None, 0, None, None, None, codes, None, None, None, None,
                                                 v, b, (1 << 32) + 64, ctypes.byref(u))
print(json.dumps(out))
'''


def test_conventions_before_init():
    from narwhal_amd import _lib
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["bound"] == 1192 and got["bound_big"] == (1 << 40) + 64 * (1 << 33), got
    assert got["null_body"] == _lib.NWC_ERR_ARG and got["null_body_code"] == _lib.NWC_ERR_ARG and got["null_body_zeroed"], got
    assert got["null_used"] == _lib.NWC_ERR_ARG, got
    assert got["cap_below"] == _lib.NWC_ERR_ARG and got["cap_below_zeroed"], got
    assert got["m0"] == 0 and got["m0_untouched"], got
    assert got["not_init"] == _lib.NWC_ERR_NOT_INIT and got["not_init_code"] == _lib.NWC_ERR_NOT_INIT, got
    assert "nwc_init" in got["not_init_text"] and got["not_init_zeroed"] and got["body_untouched"], got
    assert got["no_views"] == got["no_views_ex"] == _lib.NWC_ERR_NOT_INIT, got
    assert got["signer_null_outputs"] == _lib.NWC_ERR_ARG, got
    assert got["dev_null_body"] == _lib.NWC_ERR_ARG and got["dev_cap_below"] == _lib.NWC_ERR_ARG, got
    assert got["dev_m0"] == 0 and got["dev_not_init"] == _lib.NWC_ERR_NOT_INIT and got["dev_no_views"] == _lib.NWC_ERR_NOT_INIT, got
    assert got["codes_untouched"] and got["too_long"] == _lib.NWC_ERR_ARG, got
