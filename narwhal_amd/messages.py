"""Host-side mirror of the reference's primary messages (/root/reference/primary/src/messages.rs)
and of Core's batched sanitisation (primary/src/core.rs:306-346), backed by the GPU message
pipeline of libnwc.so (nwc_sanitize_messages: bincode + base64 decoding, Header / Vote /
Certificate digests, committee checks and all signatures on the device).

  Header       messages.rs:13-85     author, round, payload {Digest: WorkerId}, parents {Digest},
                                     id, signature; digest(); verify(committee)
  Vote         messages.rs:104-154   id, round, origin, author, signature
  Certificate  messages.rs:168-235   header, votes [(PublicKey, Signature)]; genesis(committee)
  Committee    config/src/lib.rs:134-212  authorities {PublicKey: Authority(stake, workers)}
  DagError     primary/src/error.rs  verification failures (code + variant name)
  sanitize_many(messages, committee, gc_round, current_header) -> [DagError | None]
  sanitize_many_ex(messages, committee, states, gc_round, target, signer)
                                     -> [(DagError | None, Digest, kind, Signature | None)]
  sanitize_many_view(...)            the same, plus the Header / Vote / Certificate of every message
                                     that decoded, built from the device's view of it and the wire
Wire format = bincode of `PrimaryMessage` (primary/src/primary.rs:33-38), built by `to_bytes()`.
The object-level `verify` / `digest` calls go through the same GPU batch path (a batch of one);
there is no CPU verification path.
"""
from __future__ import annotations

import base64
import ctypes
import struct
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple

from . import _lib
from .crypto import Digest, PublicKey, SecretKey, Signature, Signer, digest_bytes

__all__ = ["DagError", "Authority", "Committee", "Header", "Vote", "Certificate", "sanitize_many",
           "sanitize_many_ex", "sanitize_many_view", "Sanitizer", "DAG_ERRORS"]

DAG_ERRORS = ["Ok", "InvalidSignature", "InvalidHeaderId", "MalformedHeader", "UnknownAuthority",
              "AuthorityReuse", "CertificateRequiresQuorum", "TooOld", "SerializationError", "UnexpectedVote",
              "UnexpectedMessage", "DecodePanic"]


class DagError(Exception):
    """primary/src/error.rs DagError: `code` is the NWC_DAG_* value, `name` the variant."""

    def __init__(self, code: int):
        self.code = int(code)
        self.name = DAG_ERRORS[self.code] if 0 <= self.code < len(DAG_ERRORS) else "Unknown"
        super().__init__(self.name)


@dataclass
class Authority:
    stake: int
    workers: Sequence[int] = (0,)


class Committee:
    """config::Committee: authorities ordered as the reference's BTreeMap<PublicKey, _>."""

    def __init__(self, authorities: Dict[PublicKey, Authority]):
        self.authorities = dict(sorted(authorities.items(), key=lambda kv: bytes(kv[0])))

    def stake(self, name: PublicKey) -> int:
        a = self.authorities.get(name)
        return a.stake if a else 0

    def quorum_threshold(self) -> int:
        return 2 * sum(a.stake for a in self.authorities.values()) // 3 + 1

    def install(self) -> None:
        """Upload keys, stakes and worker ids (nwc_set_committee_config).  Every sanitize_many call
        installs its committee: another caller may have replaced the device-side committee."""
        lib = _lib.load()
        keys = b"".join(bytes(k) for k in self.authorities)
        stakes = (ctypes.c_uint64 * max(1, len(self.authorities)))(*[a.stake for a in self.authorities.values()])
        offs, ids = [0], []
        for a in self.authorities.values():
            ids.extend(int(w) for w in a.workers)
            offs.append(len(ids))
        offs_c = (ctypes.c_uint32 * len(offs))(*offs)
        ids_c = (ctypes.c_uint32 * max(1, len(ids)))(*ids)
        _lib.check(lib.nwc_set_committee_config(_lib.buf(keys) if keys else None, stakes, len(self.authorities),
                                                offs_c, ids_c))


# ---- bincode helpers -------------------------------------------------------------------------
def _key(pk: PublicKey) -> bytes:
    s = pk.encode_base64().encode()
    return struct.pack("<Q", len(s)) + s


@dataclass
class Header:
    author: PublicKey = field(default_factory=PublicKey)
    round: int = 0
    payload: Dict[Digest, int] = field(default_factory=dict)
    parents: Set[Digest] = field(default_factory=set)
    id: Digest = field(default_factory=Digest)
    signature: Signature = field(default_factory=Signature)

    @classmethod
    def new(cls, author: PublicKey, round: int, payload: Dict[Digest, int], parents: Set[Digest],
            secret: SecretKey) -> "Header":
        """Header::new (messages.rs:24-46): id = digest(), signature over the id."""
        h = cls(author, round, dict(payload), set(parents))
        h.id = h.digest()
        h.signature = Signature.new(h.id, secret)
        return h

    def digest_input(self) -> bytes:
        b = bytes(self.author) + struct.pack("<Q", self.round)
        for d in sorted(self.payload):
            b += bytes(d) + struct.pack("<I", self.payload[d])
        for p in sorted(self.parents):
            b += bytes(p)
        return b

    def digest(self) -> Digest:
        """Hash for Header (messages.rs:70-84) -- SHA-512 on the GPU."""
        return digest_bytes(self.digest_input())

    def encode(self) -> bytes:
        b = _key(self.author) + struct.pack("<Q", self.round) + struct.pack("<Q", len(self.payload))
        for d in sorted(self.payload):
            b += bytes(d) + struct.pack("<I", self.payload[d])
        b += struct.pack("<Q", len(self.parents)) + b"".join(bytes(p) for p in sorted(self.parents))
        return b + bytes(self.id) + self.signature.flatten()

    def to_bytes(self) -> bytes:
        """bincode of PrimaryMessage::Header(self)."""
        return struct.pack("<I", 0) + self.encode()

    def verify(self, committee: Committee) -> None:
        """Header::verify (messages.rs:48-67); raises DagError."""
        _raise(sanitize_many([self.to_bytes()], committee)[0])


@dataclass
class Vote:
    id: Digest
    round: int
    origin: PublicKey
    author: PublicKey
    signature: Signature = field(default_factory=Signature)

    @classmethod
    def new(cls, header: Header, author: PublicKey, secret) -> "Vote":
        """Vote::new (messages.rs:115-129).  `secret`: a SecretKey, or a Signer (a registered key:
        digest and signature in one launch, nwc_signer_vote)."""
        v = cls(header.id, header.round, header.author, author)
        if isinstance(secret, Signer):
            v.signature = secret.vote(header.id, header.round, header.author)
        else:
            v.signature = Signature.new(v.digest(), secret)
        return v

    def digest(self) -> Digest:
        """Hash for Vote (messages.rs:145-153)."""
        return digest_bytes(bytes(self.id) + struct.pack("<Q", self.round) + bytes(self.origin))

    def to_bytes(self) -> bytes:
        return (struct.pack("<I", 1) + bytes(self.id) + struct.pack("<Q", self.round) + _key(self.origin) +
                _key(self.author) + self.signature.flatten())

    def verify(self, committee: Committee) -> None:
        """Vote::verify (messages.rs:131-142); raises DagError."""
        _raise(sanitize_many([self.to_bytes()], committee)[0])


@dataclass
class Certificate:
    header: Header = field(default_factory=Header)
    votes: List[Tuple[PublicKey, Signature]] = field(default_factory=list)

    @staticmethod
    def genesis(committee: Committee) -> List["Certificate"]:
        return [Certificate(Header(author=name)) for name in committee.authorities]

    def round(self) -> int:
        return self.header.round

    def origin(self) -> PublicKey:
        return self.header.author

    def digest(self) -> Digest:
        """Hash for Certificate (messages.rs:226-234)."""
        return digest_bytes(bytes(self.header.id) + struct.pack("<Q", self.round()) + bytes(self.origin()))

    def to_bytes(self) -> bytes:
        b = struct.pack("<I", 2) + self.header.encode() + struct.pack("<Q", len(self.votes))
        for k, s in self.votes:
            b += _key(k) + s.flatten()
        return b

    def verify(self, committee: Committee) -> None:
        """Certificate::verify (messages.rs:189-215); raises DagError."""
        _raise(sanitize_many([self.to_bytes()], committee)[0])


class Sanitizer:
    """Concurrent one-message sanitize calls behind shared pipeline launches (nwc_sanitizer):
    `sanitize` blocks and answers as `sanitize_many` on that message alone, but calls made from
    several threads at once are packed into groups that one set of launches decides.  `gc_round`
    and `target` belong to the call.  A group closes at `max_messages` messages (0 = as many as
    fit), when it is full, or `max_wait_us` after it was opened (0 = never wait for company).  The
    committee is the one last installed (`Committee.install`).  A context manager; `close()` lets
    queued requests finish.  `lib`: a loaded library (tests).  `committee`: the installed committee,
    which `sanitize_view` needs to name a certificate's voters (views carry committee indices)."""

    STATS = ("groups", "messages", "bytes", "equations", "redone_messages", "bypassed_messages",
             "max_messages_in_group", "reserved")

    def __init__(self, max_messages: int = 0, max_wait_us: int = 0, lib=None, committee: Optional[Committee] = None):
        self._lib = lib if lib is not None else _lib.load()
        self.committee = committee
        self.handle = self._lib.nwc_sanitizer_create(max_messages, max_wait_us)
        if not self.handle:
            raise _lib.DeviceError("nwc_sanitizer_create failed (%d): %s" % (self._lib.nwc_last_error_code(),
                                                                             self._lib.nwc_last_error().decode()))

    def sanitize(self, wire: bytes, gc_round: int = 0, target: Optional[Header] = None) -> Tuple[int, Digest, int]:
        """(code, digest, kind) of one wire message: the NWC_DAG_* code (< 0: a device error), the
        message's digest and its kind (0 header, 1 vote, 2 certificate, 3 other)."""
        wire = bytes(wire)
        t = None
        if target is not None:
            t = bytes(target.id) + struct.pack("<Q", target.round) + bytes(target.author)
        dig = ctypes.create_string_buffer(32)
        kind = ctypes.create_string_buffer(1)
        code = self._lib.nwc_sanitizer_sanitize(self.handle, _lib.buf(wire) if wire else None, len(wire), gc_round,
                                                _lib.buf(t) if t else None, dig, kind)
        return int(code), Digest(dig.raw), kind.raw[0]

    def sanitize_vote(self, wire: bytes, signer: Signer, gc_round: int = 0,
                      target: Optional[Header] = None) -> Tuple[int, Digest, int, Optional[Signature]]:
        """`sanitize`, and for a header whose code is Ok the signature of Vote::new(header, ..) under
        `signer`'s key from the same flight (nwc_sanitizer_sanitize_vote); None otherwise.  The
        library keeps no voting state: Core's last_voted check stays with the caller."""
        wire = bytes(wire)
        t = None
        if target is not None:
            t = bytes(target.id) + struct.pack("<Q", target.round) + bytes(target.author)
        dig = ctypes.create_string_buffer(32)
        kind = ctypes.create_string_buffer(1)
        sig = ctypes.create_string_buffer(64)
        voted = ctypes.c_int32(0)
        code = self._lib.nwc_sanitizer_sanitize_vote(self.handle, signer.handle, _lib.buf(wire) if wire else None,
                                                     len(wire), gc_round, _lib.buf(t) if t else None, dig, kind, sig,
                                                     ctypes.byref(voted))
        return int(code), Digest(dig.raw), kind.raw[0], Signature.from_bytes(sig.raw) if voted.value else None

    def vote_stats(self) -> dict:
        """Votes signed inside a group flight / by the one-message fallback."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(self._lib.nwc_sanitizer_vote_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return {"in_flight": int(a.value), "alone": int(b.value)}

    def sanitize_view(self, wire: bytes, gc_round: int = 0, target: Optional[Header] = None,
                      signer: Optional[Signer] = None) -> tuple:
        """`sanitize_vote`'s tuple (the signature None without a signer) plus the Header / Vote /
        Certificate the device decoded in the same flight (nwc_sanitizer_sanitize_view), built by
        `_view_objects` from the record, the wire and the body; None for a message that did not
        decode.  A certificate's voters are named through `committee` (the constructor's)."""
        wire = bytes(wire)
        t = _target72(target)
        dig = ctypes.create_string_buffer(32)
        kind = ctypes.create_string_buffer(1)
        sig = ctypes.create_string_buffer(64) if signer is not None else None
        voted = ctypes.c_int32(0)
        view = _lib.MsgView()
        cap = int(self._lib.nwc_msg_view_body_bound(len(wire), 1))
        body = ctypes.create_string_buffer(cap)
        used = ctypes.c_uint64(0)
        code = self._lib.nwc_sanitizer_sanitize_view(self.handle, signer.handle if signer is not None else None,
                                                     _lib.buf(wire) if wire else None, len(wire), gc_round,
                                                     _lib.buf(t) if t else None, dig, kind, sig,
                                                     ctypes.byref(voted) if signer is not None else None,
                                                     ctypes.byref(view), body, cap, ctypes.byref(used))
        obj = None
        if code >= 0 and view.decoded:
            if view.n_votes and self.committee is None:
                raise ValueError("Sanitizer(committee=...) is needed to name a certificate's voters")
            keys = list(self.committee.authorities) if self.committee is not None else []
            obj = _view_objects(view, wire, body.raw[:used.value], keys)
        return (int(code), Digest(dig.raw), kind.raw[0],
                Signature.from_bytes(sig.raw) if signer is not None and voted.value else None, obj)

    def view_stats(self) -> dict:
        """Views delivered by a group flight / by the one-message fallback."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(self._lib.nwc_sanitizer_view_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return {"in_flight": int(a.value), "alone": int(b.value)}

    def check(self, wire: bytes, gc_round: int = 0, target: Optional[Header] = None) -> Tuple[Digest, int]:
        """`sanitize`, raising DagError for a code > 0 and DeviceError for a code < 0; (digest, kind)."""
        code, dig, kind = self.sanitize(wire, gc_round, target)
        if code < 0:
            raise _lib.DeviceError("libnwc error %d: %s" % (code, self._lib.nwc_last_error().decode()))
        if code != 0:
            raise DagError(code)
        return dig, kind

    def stats(self) -> dict:
        out = (ctypes.c_uint64 * len(self.STATS))()
        _lib.check(self._lib.nwc_sanitizer_stats(self.handle, out))
        return {k: int(v) for k, v in zip(self.STATS, out)}

    def close(self) -> None:
        if self.handle:
            h, self.handle = self.handle, None
            _lib.check(self._lib.nwc_sanitizer_destroy(h))

    def __enter__(self) -> "Sanitizer":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter teardown)
            pass


def _raise(err: Optional[DagError]) -> None:
    if err is not None:
        raise err


def sanitize_many(messages: Sequence[bytes], committee: Committee, gc_round: int = 0,
                  current_header: Optional[Header] = None, digests: Optional[list] = None) -> List[Optional[DagError]]:
    """Core::sanitize_header / sanitize_vote / sanitize_certificate over a batch of wire messages
    (bincode PrimaryMessage bytes, as PrimaryReceiverHandler::dispatch receives them).  Returns
    None (Ok) or the DagError per message; `digests` (a list) receives each message's digest."""
    lib = _lib.load()
    committee.install()
    m = len(messages)
    if m == 0:
        return []
    offs = [0]
    for b in messages:
        offs.append(offs[-1] + len(b))
    data = b"".join(messages) or b"\0"
    offsets = (ctypes.c_uint64 * (m + 1))(*offs)
    codes = (ctypes.c_int32 * m)()
    dig = ctypes.create_string_buffer(32 * m) if digests is not None else None
    target = None
    if current_header is not None:
        target = bytes(current_header.id) + struct.pack("<Q", current_header.round) + bytes(current_header.author)
    _lib.check(lib.nwc_sanitize_messages(_lib.buf(data), offsets, m, gc_round, _lib.buf(target) if target else None,
                                         codes, dig, None))
    if digests is not None:
        raw = dig.raw   # one copy (`.raw` copies the whole buffer on every access)
        digests.extend(Digest(raw[32 * i:32 * i + 32]) for i in range(m))
    return [None if c == 0 else DagError(c) for c in codes]


def _target72(h: Optional[Header]) -> Optional[bytes]:
    return None if h is None else bytes(h.id) + struct.pack("<Q", h.round) + bytes(h.author)


def sanitize_many_ex(messages: Sequence[bytes], committee: Committee,
                     states: Optional[Sequence[Tuple[int, Optional[Header]]]] = None, gc_round: int = 0,
                     target: Optional[Header] = None,
                     signer: Optional[Signer] = None) -> List[Tuple[Optional[DagError], Digest, int, Optional[Signature]]]:
    """`sanitize_many` with Core's state per message and Vote::new from the same call
    (nwc_sanitize_messages_ex).  `states`: per message the (gc_round, current header or None) that
    held when the frame was received; None judges every message under `gc_round` and `target`.
    `signer`: a registered key; every header whose verdict is Ok then comes back with the signature
    of Vote::new(header, signer's key).  Returns per message (DagError or None, digest, kind,
    Signature or None).  The library keeps no voting state: Core's last_voted check stays with the
    caller."""
    lib = _lib.load()
    committee.install()
    m = len(messages)
    if m == 0:
        return []
    if states is not None and len(states) != m:
        raise ValueError("states: one (gc_round, current header) per message")
    offs = [0]
    for b in messages:
        offs.append(offs[-1] + len(b))
    data = b"".join(messages) or b"\0"
    offsets = (ctypes.c_uint64 * (m + 1))(*offs)
    codes = (ctypes.c_int32 * m)()
    dig = ctypes.create_string_buffer(32 * m)
    kinds = ctypes.create_string_buffer(m)
    gcs = recs = None
    if states is not None:
        gcs = (ctypes.c_uint64 * m)(*[int(s[0]) for s in states])
        # the 80-byte record: id, round LE, origin, the "enabled" byte, seven zero bytes
        recs = b"".join(bytes(80) if s[1] is None else _target72(s[1]) + b"\x01" + bytes(7) for s in states)
    sigs = ctypes.create_string_buffer(64 * m) if signer is not None else None
    voted = ctypes.create_string_buffer(m) if signer is not None else None
    t = _target72(target)
    _lib.check(lib.nwc_sanitize_messages_ex(_lib.buf(data), offsets, m, gcs, gc_round, _lib.buf(recs) if recs else None,
                                            _lib.buf(t) if t else None, signer.handle if signer is not None else None,
                                            codes, dig, kinds, sigs, voted))
    raw, kraw = dig.raw, kinds.raw
    sraw, vraw = (sigs.raw, voted.raw) if signer is not None else (b"", bytes(m))
    return [(None if codes[i] == 0 else DagError(codes[i]), Digest(raw[32 * i:32 * i + 32]), kraw[i],
             Signature.from_bytes(sraw[64 * i:64 * i + 64]) if vraw[i] else None) for i in range(m)]


def _view_objects(v: "_lib.MsgView", wire: bytes, body: bytes, keys: List[PublicKey]):
    """Header / Vote / Certificate of one decoded message from its view, the wire and the body."""
    sig = Signature.from_bytes(wire[v.sig_off:v.sig_off + 64])
    if v.kind == 1:
        return Vote(Digest(bytes(v.id)), int(v.round), PublicKey(bytes(v.origin)), PublicKey(bytes(v.author)), sig)
    src, at = (body, v.payload_off) if v.flags & _lib.VIEW_PAYLOAD_IN_BODY else (wire, v.payload_off)
    payload = {Digest(src[at + 36 * e:at + 36 * e + 32]): struct.unpack_from("<I", src, at + 36 * e + 32)[0]
               for e in range(v.n_payload)}
    src, at = (body, v.parents_off) if v.flags & _lib.VIEW_PARENTS_IN_BODY else (wire, v.parents_off)
    parents = {Digest(src[at + 32 * e:at + 32 * e + 32]) for e in range(v.n_parents)}
    header = Header(PublicKey(bytes(v.author)), int(v.round), payload, parents, Digest(bytes(v.id)), sig)
    if v.kind == 0:
        return header
    votes = []
    for e in range(v.n_votes):
        k, off = struct.unpack_from("<iI", body, v.votes_off + 8 * e)
        n = struct.unpack_from("<Q", wire, off)[0]
        if k >= 0:
            key = keys[k]
        else:
            # a voter outside the committee: the key is the first 32 bytes its text encodes (the
            # device has accepted the text: 43 symbols of the alphabet come first)
            key = PublicKey(base64.b64decode(wire[off + 8:off + 8 + 43] + b"=")[:32])
        votes.append((key, Signature.from_bytes(wire[off + 8 + n:off + 8 + n + 64])))
    return Certificate(header, votes)


def sanitize_many_view(messages: Sequence[bytes], committee: Committee,
                       states: Optional[Sequence[Tuple[int, Optional[Header]]]] = None, gc_round: int = 0,
                       target: Optional[Header] = None, signer: Optional[Signer] = None) -> List[tuple]:
    """`sanitize_many_ex` that also hands back what the device decoded (nwc_sanitize_messages_view).
    Returns per message (DagError or None, digest, kind, Signature or None, object): `object` is the
    Header / Vote / Certificate of a message that decoded -- whatever its verdict -- built from its
    view and the wire bytes alone, and None for one that did not (SerializationError,
    UnexpectedMessage, DecodePanic).  Nothing is decoded on the host: fields come from the record,
    payload and parents from the wire or the body at the offsets the record names, voters from the
    committee by index (only a voter outside the committee has its key text read)."""
    lib = _lib.load()
    committee.install()
    m = len(messages)
    if m == 0:
        return []
    if states is not None and len(states) != m:
        raise ValueError("states: one (gc_round, current header) per message")
    offs = [0]
    for b in messages:
        offs.append(offs[-1] + len(b))
    data = b"".join(messages) or b"\0"
    offsets = (ctypes.c_uint64 * (m + 1))(*offs)
    codes = (ctypes.c_int32 * m)()
    dig = ctypes.create_string_buffer(32 * m)
    kinds = ctypes.create_string_buffer(m)
    gcs = recs = None
    if states is not None:
        gcs = (ctypes.c_uint64 * m)(*[int(s[0]) for s in states])
        recs = b"".join(bytes(80) if s[1] is None else _target72(s[1]) + b"\x01" + bytes(7) for s in states)
    sigs = ctypes.create_string_buffer(64 * m) if signer is not None else None
    voted = ctypes.create_string_buffer(m) if signer is not None else None
    views = (_lib.MsgView * m)()
    cap = int(lib.nwc_msg_view_body_bound(offs[-1], m))
    body = ctypes.create_string_buffer(cap)
    used = ctypes.c_uint64(0)
    t = _target72(target)
    _lib.check(lib.nwc_sanitize_messages_view(_lib.buf(data), offsets, m, gcs, gc_round, _lib.buf(recs) if recs else None,
                                              _lib.buf(t) if t else None, signer.handle if signer is not None else None,
                                              codes, dig, kinds, sigs, voted, views, body, cap, ctypes.byref(used)))
    raw, kraw = dig.raw, kinds.raw
    sraw, vraw = (sigs.raw, voted.raw) if signer is not None else (b"", bytes(m))
    braw = body.raw[:used.value]
    keys = list(committee.authorities)
    return [(None if codes[i] == 0 else DagError(codes[i]), Digest(raw[32 * i:32 * i + 32]), kraw[i],
             Signature.from_bytes(sraw[64 * i:64 * i + 64]) if vraw[i] else None,
             _view_objects(views[i], bytes(messages[i]), braw, keys) if views[i].decoded else None) for i in range(m)]
