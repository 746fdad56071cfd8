"""A small model of nwc_msg_view (include/nwc.h) -- TEST INFRASTRUCTURE ONLY.

expected(msg, keys, code) is what nwc_sanitize_messages_view must report for one wire message: the
decoded fields come from oracle/messages_ref.py `decode` (canonical payload and parents, decoded
keys, the vote list; imported read-only), the offsets from one walk over the wire.  pack() lays the
expected views of a batch out as the library would (records + a body whose areas are handed out in
message order) and rebuild() goes the other way: from (record, wire, body, committee keys) alone to
the object `decode` yields, reading the wire only at the offsets the record names.
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

import messages_ref as mr  # noqa: E402

PAYLOAD_IN_BODY, PARENTS_IN_BODY = 1, 2
RECORD = struct.Struct("<BBBBiQ32s32s32siiIIIIQQQ")
FIELDS = ("decoded", "kind", "flags", "reserved0", "code", "round", "author", "origin", "id", "author_index",
          "origin_index", "n_payload", "n_parents", "n_votes", "sig_off", "payload_off", "parents_off", "votes_off")
assert RECORD.size == 160
# byte offset of every field, as the header's struct lays them out
OFFSETS = dict(decoded=0, kind=1, flags=2, reserved0=3, code=4, round=8, author=16, origin=48, id=80, author_index=112,
               origin_index=116, n_payload=120, n_parents=124, n_votes=128, sig_off=132, payload_off=136, parents_off=144,
               votes_off=152)


def body_bound(total, m):
    return total + 64 * m


def _u64(b, p):
    return struct.unpack_from("<Q", b, p)[0]


def _index(keys, k):
    return keys.index(k) if k in keys else -1


def _ascending(entries):
    return all(a < b for a, b in zip(entries, entries[1:]))


def expected(msg, keys, code):
    """The view of one message as a dict: FIELDS, with payload_off / parents_off None where the
    entries are in the body, plus `payload` [(digest, worker id)], `parents` [digest] (canonical)
    and `votes` [(member index, vote offset)].  keys: the committee in configuration order."""
    kind, f = mr.decode(msg)
    v = dict.fromkeys(FIELDS, 0)
    v.update(code=code, author=bytes(32), origin=bytes(32), id=bytes(32), payload=[], parents=[], votes=[])
    if kind not in (0, 1, 2):
        # the kind of a message that failed to decode is the variant it announced, as kinds[i]
        variant = struct.unpack_from("<I", msg)[0] if len(msg) >= 4 else 3
        v["kind"] = variant if variant <= 2 else 3
        return v
    v.update(decoded=1, kind=kind)
    if kind == 1:
        p = 4 + 32 + 8
        p += 8 + _u64(msg, p)
        p += 8 + _u64(msg, p)
        v.update(round=f["round"], author=f["author"], origin=f["origin"], id=f["id"], sig_off=p,
                 author_index=_index(keys, f["author"]), origin_index=_index(keys, f["origin"]))
        return v
    h = f if kind == 0 else f["header"]
    p = 4
    p += 8 + _u64(msg, p) + 8
    P = _u64(msg, p)
    pay = p + 8
    p = pay + 36 * P
    Q = _u64(msg, p)
    par = p + 8
    p = par + 32 * Q + 32
    wire_payload = [msg[pay + 36 * e:pay + 36 * e + 32] for e in range(P)]
    wire_parents = [msg[par + 32 * e:par + 32 * e + 32] for e in range(Q)]
    flags = (0 if _ascending(wire_payload) else PAYLOAD_IN_BODY) | (0 if _ascending(wire_parents) else PARENTS_IN_BODY)
    v.update(round=h["round"], author=h["author"], id=h["id"], sig_off=p, author_index=_index(keys, h["author"]),
             origin_index=-1, flags=flags, n_payload=len(h["payload"]), n_parents=len(h["parents"]),
             payload=list(h["payload"]), parents=list(h["parents"]),
             payload_off=None if flags & PAYLOAD_IN_BODY else pay, parents_off=None if flags & PARENTS_IN_BODY else par)
    if kind == 2:
        p += 64
        V = _u64(msg, p)
        p += 8
        assert V == len(f["votes"])
        for key, _ in f["votes"]:
            v["votes"].append((_index(keys, key), p))
            p += 8 + _u64(msg, p) + 64
        v["n_votes"] = V
    return v


def _al16(n):
    return (n + 15) & ~15


def pack(views):
    """The records (160 bytes each) and the body of a batch of expected views, areas in message order."""
    recs, body = [], bytearray()
    for v in views:
        v = dict(v)
        if v["decoded"] and v["kind"] != 1:
            if v["payload_off"] is None:
                v["payload_off"] = len(body)
                body += b"".join(d + struct.pack("<I", w) for d, w in v["payload"])
                body += bytes(_al16(len(body)) - len(body))
            if v["parents_off"] is None:
                v["parents_off"] = len(body)
                body += b"".join(v["parents"])
                body += bytes(_al16(len(body)) - len(body))
            if v["votes"]:
                v["votes_off"] = len(body)
                body += b"".join(struct.pack("<iI", k, off) for k, off in v["votes"])
                body += bytes(_al16(len(body)) - len(body))
        recs.append(RECORD.pack(*[v[k] for k in FIELDS]))
    return b"".join(recs), bytes(body)


def unpack(rec):
    return dict(zip(FIELDS, RECORD.unpack(rec)))


def areas(v):
    """[(offset, length)] of the body areas a record names"""
    out = []
    if v["decoded"] and v["flags"] & PAYLOAD_IN_BODY:
        out.append((v["payload_off"], 36 * v["n_payload"]))
    if v["decoded"] and v["flags"] & PARENTS_IN_BODY:
        out.append((v["parents_off"], 32 * v["n_parents"]))
    if v["decoded"] and v["n_votes"]:
        out.append((v["votes_off"], 8 * v["n_votes"]))
    return out


def entries(v, wire, body):
    """(payload, parents, votes) that a record names in the wire / the body"""
    src, at = (body, v["payload_off"]) if v["flags"] & PAYLOAD_IN_BODY else (wire, v["payload_off"])
    payload = [(bytes(src[at + 36 * e:at + 36 * e + 32]), struct.unpack_from("<I", src, at + 36 * e + 32)[0])
               for e in range(v["n_payload"])]
    src, at = (body, v["parents_off"]) if v["flags"] & PARENTS_IN_BODY else (wire, v["parents_off"])
    parents = [bytes(src[at + 32 * e:at + 32 * e + 32]) for e in range(v["n_parents"])]
    votes = [struct.unpack_from("<iI", body, v["votes_off"] + 8 * e) for e in range(v["n_votes"])]
    return payload, parents, votes


def rebuild(rec, wire, body, keys):
    """mr.decode's (kind, fields) from a record, the wire and the body alone; (None, None) for a
    message that did not decode.  Only a voter outside the committee has its key text decoded."""
    v = unpack(rec) if isinstance(rec, (bytes, bytearray)) else rec
    if not v["decoded"]:
        return None, None
    sig = bytes(wire[v["sig_off"]:v["sig_off"] + 64])
    if v["kind"] == 1:
        return 1, dict(id=v["id"], round=v["round"], origin=v["origin"], author=v["author"], sig=sig)
    payload, parents, votes = entries(v, wire, body)
    h = dict(author=v["author"], round=v["round"], payload=payload, parents=parents, id=v["id"], sig=sig)
    if v["kind"] == 0:
        return 0, h
    out = []
    for k, off in votes:
        n = _u64(wire, off)
        key = keys[k] if k >= 0 else mr.b64_013_decode(bytes(wire[off + 8:off + 8 + n]))[:32]
        out.append((key, bytes(wire[off + 8 + n:off + 8 + n + 64])))
    return 2, dict(header=h, votes=out)


def check_against(got_rec, got_body, body_used, exp, wire, what=""):
    """One library record against the model's view: every fixed field, wire offsets where the entries
    stay in the wire, and the contents of every area the record names."""
    g = unpack(got_rec)
    for k in FIELDS:
        if k in ("payload_off", "parents_off", "votes_off"):
            continue
        assert g[k] == exp[k], (what, k, g[k], exp[k])
    if not g["decoded"]:
        assert bytes(got_rec[8:]) == bytes(152) and g["flags"] == 0 and g["reserved0"] == 0, what
        return g
    if g["kind"] == 1:
        assert (g["payload_off"], g["parents_off"], g["votes_off"]) == (0, 0, 0), what
        return g
    for k in ("payload_off", "parents_off"):
        if exp[k] is not None:
            assert g[k] == exp[k], (what, k, g[k], exp[k])
    for at, n in areas(g):
        assert at % 16 == 0 and at + n <= body_used, (what, at, n, body_used)
    if not g["n_votes"]:
        assert g["votes_off"] == 0, what
    payload, parents, votes = entries(g, wire, got_body)
    assert payload == exp["payload"], what
    assert parents == exp["parents"], what
    assert [tuple(x) for x in votes] == exp["votes"], what
    return g


def check_disjoint(recs, body_used):
    """The areas of a call's records: 16-aligned, inside [0, body_used), pairwise disjoint."""
    spans = sorted(a for r in recs for a in areas(r) if a[1])
    for (a0, n0), (a1, _) in zip(spans, spans[1:]):
        assert a0 + n0 <= a1, (a0, n0, a1)
    for at, n in spans:
        assert at % 16 == 0 and at + n <= body_used
