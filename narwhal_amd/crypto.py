"""Host-side mirror of the reference's `crypto` crate (/root/reference/crypto/src/lib.rs),
backed by the MI355X kernels in libnwc.so.

Same names, argument meaning and error behaviour as the Rust API, so that parity tests read
like crypto/src/tests/crypto_tests.rs:
  Digest            lib.rs:20-57     32-byte digest, Debug/Display = base64
  Hash              lib.rs:59-62     `digest()`; `Hash for &[u8]` = SHA-512[..32] (tests :8-12)
  PublicKey         lib.rs:64-118    32 bytes, serde as base64
  SecretKey         lib.rs:120-161   64 bytes (seed || public), zeroised on drop
  generate_keypair  lib.rs:167-175
  Signature         lib.rs:177-219   new / verify / verify_batch, Default = 64 zero bytes
  SignatureService  lib.rs:222-250   request_signature; a Signer is the registered key behind it
  CryptoError       lib.rs:18        opaque verification failure (Rust `Err`)
Device/runtime failures raise `DeviceError` -- never `CryptoError`.
Verification, hashing and signing all run on the GPU; there is no CPU path here.
"""
from __future__ import annotations

import base64
import ctypes
import os
import threading
from typing import Iterable, Optional, Sequence, Tuple

from . import _lib
from ._lib import DeviceError

__all__ = ["CryptoError", "DeviceError", "Digest", "Hash", "PublicKey", "SecretKey", "Signature",
           "generate_keypair", "generate_production_keypair", "digest_bytes", "digest_many", "Signer",
           "SignatureService", "keypair_from_seed", "Verifier"]


class CryptoError(Exception):
    """`pub type CryptoError = ed25519::Error` -- an opaque verification failure."""


class Digest:
    __slots__ = ("_b",)

    def __init__(self, b: bytes = bytes(32)):
        b = bytes(b)
        if len(b) != 32:
            raise ValueError("Digest must be 32 bytes")
        self._b = b

    @classmethod
    def try_from(cls, item: bytes) -> "Digest":
        return cls(item)

    def to_vec(self) -> bytes:
        return self._b

    def size(self) -> int:
        return 32

    def __bytes__(self) -> bytes:
        return self._b

    def __eq__(self, o) -> bool:
        return isinstance(o, Digest) and o._b == self._b

    def __lt__(self, o) -> bool:
        return self._b < o._b

    def __hash__(self) -> int:
        return hash(self._b)

    def __repr__(self) -> str:  # Debug = base64 (lib.rs:34-38)
        return base64.b64encode(self._b).decode()

    def __str__(self) -> str:  # Display = first 16 base64 chars (lib.rs:40-44)
        return base64.b64encode(self._b).decode()[:16]


class Hash:
    """`pub trait Hash { fn digest(&self) -> Digest; }`"""

    def digest(self) -> Digest:  # pragma: no cover - interface
        raise NotImplementedError


def digest_bytes(data: bytes) -> Digest:
    """`impl Hash for &[u8]`: Digest(Sha512::digest(data)[..32]) -- on the GPU."""
    lib = _lib.load()
    out = ctypes.create_string_buffer(32)
    data = bytes(data)
    _lib.check(lib.nwc_digest32(_lib.buf(data) if data else None, len(data), out))
    return Digest(out.raw)


def digest_many(messages: Sequence[bytes]) -> list:
    """Batched worker digests (worker/src/processor.rs:38) for many serialized batches."""
    lib = _lib.load()
    offs = [0]
    for m in messages:
        offs.append(offs[-1] + len(m))
    data = b"".join(messages)
    offsets = (ctypes.c_uint64 * len(offs))(*offs)
    out = ctypes.create_string_buffer(32 * len(messages))
    _lib.check(lib.nwc_sha512_trunc32_many(_lib.buf(data) if data else None, offsets, len(messages), out))
    raw = out.raw
    return [Digest(raw[32 * i:32 * i + 32]) for i in range(len(messages))]


class PublicKey:
    __slots__ = ("_b",)

    def __init__(self, b: bytes = bytes(32)):
        b = bytes(b)
        if len(b) != 32:
            raise ValueError("PublicKey must be 32 bytes")
        self._b = b

    def encode_base64(self) -> str:
        return base64.b64encode(self._b).decode()

    @classmethod
    def decode_base64(cls, s: str) -> "PublicKey":
        raw = base64.b64decode(s, validate=True)
        if len(raw) < 32:
            raise ValueError("InvalidLength")
        return cls(raw[:32])

    def __bytes__(self) -> bytes:
        return self._b

    def __eq__(self, o) -> bool:
        return isinstance(o, PublicKey) and o._b == self._b

    def __lt__(self, o) -> bool:
        return self._b < o._b

    def __hash__(self) -> int:
        return hash(self._b)

    def __repr__(self) -> str:
        return self.encode_base64()

    def __str__(self) -> str:
        return self.encode_base64()[:16]


class SecretKey:
    """64 bytes = dalek Keypair::to_bytes() = seed || public key."""
    __slots__ = ("_b",)

    def __init__(self, b: bytes):
        b = bytearray(b)
        if len(b) != 64:
            raise ValueError("SecretKey must be 64 bytes")
        self._b = b

    def encode_base64(self) -> str:
        return base64.b64encode(bytes(self._b)).decode()

    @classmethod
    def decode_base64(cls, s: str) -> "SecretKey":
        raw = base64.b64decode(s, validate=True)
        if len(raw) < 64:
            raise ValueError("InvalidLength")
        return cls(raw[:64])

    def seed(self) -> bytes:
        return bytes(self._b[:32])

    def __eq__(self, o) -> bool:
        return isinstance(o, SecretKey) and bytes(o._b) == bytes(self._b)

    def __del__(self):
        for i in range(len(self._b)):
            self._b[i] = 0


def _keygen_sign(seeds: bytes, msgs: bytes, n: int) -> Tuple[bytes, bytes]:
    """RFC 8032 keygen + sign of n (seed, 32-byte msg) pairs on the GPU (k_keygen_sign)."""
    from . import device
    return device.keygen_sign_host(seeds, msgs, n)


def generate_keypair(rng) -> Tuple[PublicKey, SecretKey]:
    """`generate_keypair(csprng)`: 32 seed bytes from rng (dalek Keypair::generate)."""
    if hasattr(rng, "fill_bytes"):
        seed = rng.fill_bytes(32)
    elif hasattr(rng, "randbytes"):
        seed = rng.randbytes(32)
    else:
        seed = bytes(rng(32))
    pk, _ = _keygen_sign(seed, bytes(32), 1)
    return PublicKey(pk), SecretKey(seed + pk)


def generate_production_keypair() -> Tuple[PublicKey, SecretKey]:
    return generate_keypair(os.urandom)


class Signature:
    """`Signature { part1: R (32 B), part2: s (32 B) }`; Default = 64 zero bytes."""
    __slots__ = ("part1", "part2")

    def __init__(self, part1: bytes = bytes(32), part2: bytes = bytes(32)):
        if len(part1) != 32 or len(part2) != 32:
            raise ValueError("Unexpected signature length")
        self.part1 = bytes(part1)
        self.part2 = bytes(part2)

    @classmethod
    def default(cls) -> "Signature":
        return cls()

    @classmethod
    def from_bytes(cls, b: bytes) -> "Signature":
        return cls(b[:32], b[32:64])

    @classmethod
    def new(cls, digest: Digest, secret: SecretKey) -> "Signature":
        """`Signature::new(digest, secret)` = dalek sign over the 32 digest bytes (GPU)."""
        _, sig = _keygen_sign(secret.seed(), digest.to_vec(), 1)
        return cls.from_bytes(sig)

    def flatten(self) -> bytes:
        return self.part1 + self.part2

    def verify(self, digest: Digest, public_key: PublicKey) -> None:
        """`Signature::verify` -> dalek verify_strict. Raises CryptoError on an invalid signature."""
        lib = _lib.load()
        rc = _lib.check(lib.nwc_verify_strict(_lib.buf(digest.to_vec()), _lib.buf(bytes(public_key)),
                                              _lib.buf(self.flatten())))
        if rc != _lib.NWC_OK:
            raise CryptoError("signature verification failed")

    @staticmethod
    def verify_batch(digest: Digest, votes: Iterable[Tuple[PublicKey, "Signature"]],
                     bad: Optional[list] = None) -> None:
        """`Signature::verify_batch(digest, votes)`. Raises CryptoError if any vote fails.
        If `bad` is a list, it receives the indices of the failing votes (bisection result)."""
        votes = list(votes)
        lib = _lib.load()
        n = len(votes)
        pks = b"".join(bytes(p) for p, _ in votes)
        sigs = b"".join(s.flatten() for _, s in votes)
        bitmap = ctypes.create_string_buffer((n + 7) // 8 or 1)
        rc = _lib.check(lib.nwc_verify_batch(_lib.buf(digest.to_vec()), _lib.buf(pks) if n else None,
                                             _lib.buf(sigs) if n else None, n, bitmap))
        if bad is not None:
            raw = bitmap.raw
            bad.extend(i for i in range(n) if (raw[i >> 3] >> (i & 7)) & 1)
        if rc != _lib.NWC_OK:
            raise CryptoError("batch verification failed")

    def __eq__(self, o) -> bool:
        return isinstance(o, Signature) and o.flatten() == self.flatten()

    def __repr__(self) -> str:
        return "Signature { part1: %s, part2: %s }" % (list(self.part1), list(self.part2))


def _secret_bytes(secret) -> bytes:
    return bytes(secret._b) if isinstance(secret, SecretKey) else bytes(secret)


def keypair_from_seed(seed: bytes) -> Tuple[PublicKey, SecretKey]:
    """nwc_keypair_from_seed: (A, seed || A) for 32 seed bytes of the caller's CSPRNG."""
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    lib = _lib.load()
    out = ctypes.create_string_buffer(64)
    _lib.check(lib.nwc_keypair_from_seed(_lib.buf(bytes(seed)), out))
    return PublicKey(out.raw[32:]), SecretKey(out.raw)


def _vote_field(x) -> bytes:
    """The 32 bytes of a Digest, a PublicKey or a bytes-like (a vote's id or origin)."""
    b = x.to_vec() if isinstance(x, Digest) else bytes(x)
    if len(b) != 32:
        raise ValueError("a vote's id and origin must be 32 bytes")
    return b


class Signer:
    """A registered signing key (nwc_signer): the key is expanded once into device memory and every
    signature after that is one launch of a sign kernel.  A context manager; `close()` (or leaving
    the `with` block) zeroes and frees the device copy.  Raises DeviceError for a secret whose
    public half is not the seed's (a deliberate deviation from dalek's Keypair::from_bytes)."""

    def __init__(self, secret):
        b = _secret_bytes(secret)
        if len(b) != 64:
            raise ValueError("SecretKey must be 64 bytes")
        self._lib = _lib.load()
        self.handle = self._lib.nwc_signer_create(_lib.buf(b))
        if not self.handle:
            raise DeviceError("nwc_signer_create failed (%d): %s" % (self._lib.nwc_last_error_code(),
                                                                     self._lib.nwc_last_error().decode()))

    def public_key(self) -> PublicKey:
        out = ctypes.create_string_buffer(32)
        _lib.check(self._lib.nwc_signer_public_key(self.handle, out))
        return PublicKey(out.raw)

    def sign(self, digest) -> "Signature":
        """`Signature::new(digest, secret)` with the registered key."""
        d = digest.to_vec() if isinstance(digest, Digest) else bytes(digest)
        if len(d) != 32:
            raise ValueError("Digest must be 32 bytes")
        out = ctypes.create_string_buffer(64)
        _lib.check(self._lib.nwc_signer_sign(self.handle, _lib.buf(d), out))
        return Signature.from_bytes(out.raw)

    def sign_many(self, digests: Sequence) -> list:
        """One launch for all of `digests` (a round's votes)."""
        ds = [d.to_vec() if isinstance(d, Digest) else bytes(d) for d in digests]
        if any(len(d) != 32 for d in ds):
            raise ValueError("Digest must be 32 bytes")
        n = len(ds)
        if n == 0:
            return []
        out = ctypes.create_string_buffer(64 * n)
        _lib.check(self._lib.nwc_signer_sign_many(self.handle, _lib.buf(b"".join(ds)), n, out))
        raw = out.raw
        return [Signature.from_bytes(raw[64 * i:64 * i + 64]) for i in range(n)]

    def vote(self, id, round: int, origin) -> "Signature":
        """`Vote::new(header, ..)`'s signature (messages.rs:115-129) for a header the caller has
        accepted: the signature of SHA-512(id || round LE || origin)[..32], digest and signature
        in one launch (nwc_signer_vote)."""
        i, o = _vote_field(id), _vote_field(origin)
        out = ctypes.create_string_buffer(64)
        _lib.check(self._lib.nwc_signer_vote(self.handle, _lib.buf(i), int(round), _lib.buf(o), out))
        return Signature.from_bytes(out.raw)

    def vote_many(self, votes: Sequence) -> list:
        """One launch for all of `votes`, a sequence of (id, round, origin) (nwc_signer_vote_many)."""
        votes = list(votes)
        n = len(votes)
        if n == 0:
            return []
        ids = b"".join(_vote_field(v[0]) for v in votes)
        origins = b"".join(_vote_field(v[2]) for v in votes)
        rounds = (ctypes.c_uint64 * n)(*[int(v[1]) for v in votes])
        out = ctypes.create_string_buffer(64 * n)
        _lib.check(self._lib.nwc_signer_vote_many(self.handle, _lib.buf(ids), rounds, _lib.buf(origins), n, out))
        raw = out.raw
        return [Signature.from_bytes(raw[64 * i:64 * i + 64]) for i in range(n)]

    def close(self) -> None:
        if self.handle:
            h, self.handle = self.handle, None
            _lib.check(self._lib.nwc_signer_destroy(h))

    def __enter__(self) -> "Signer":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter teardown)
            pass


class SignatureService:
    """`SignatureService` (lib.rs:222-250): `request_signature(digest)` blocks until the signature
    is there.  One worker thread drains every request queued so far into one `sign_many` launch;
    requests that arrive while a launch is in flight go out together in the next one.  `signer`
    (anything with `sign_many(list of digests) -> list of Signatures`) replaces the GPU signer, so
    the queue can be exercised without a device; a signer the service created is closed by
    `close()`."""

    def __init__(self, secret=None, signer=None):
        self._own = signer is None
        self._signer = Signer(secret) if signer is None else signer
        self._cv = threading.Condition()
        self._queue = []          # [digest, result slot]
        self._closed = False
        self._requests = 0
        self._launches = 0
        self._thread = threading.Thread(target=self._run, name="nwc-signature-service", daemon=True)
        self._thread.start()

    def _run(self) -> None:
        while True:
            with self._cv:
                while not self._queue and not self._closed:
                    self._cv.wait()
                if not self._queue:
                    return
                batch, self._queue = self._queue, []
                self._launches += 1
            try:
                sigs = self._signer.sign_many([d for d, _ in batch])
                if len(sigs) != len(batch):
                    raise DeviceError("sign_many returned %d signatures for %d digests" % (len(sigs), len(batch)))
                for (_, slot), sig in zip(batch, sigs):
                    slot["sig"] = sig
            except Exception as e:  # noqa: BLE001  (handed to every waiting caller)
                for _, slot in batch:
                    slot["err"] = e
            for _, slot in batch:
                slot["done"].set()

    def request_signature(self, digest) -> "Signature":
        slot = {"done": threading.Event()}
        with self._cv:
            if self._closed:
                raise DeviceError("SignatureService is closed")
            self._queue.append((digest, slot))
            self._requests += 1
            self._cv.notify()
        slot["done"].wait()
        if "err" in slot:
            raise slot["err"]
        return slot["sig"]

    def stats(self) -> dict:
        with self._cv:
            return {"requests": self._requests, "launches": self._launches}

    def close(self) -> None:
        """Signs what is queued, stops the worker and closes a signer the service created."""
        with self._cv:
            self._closed = True
            self._cv.notify()
        self._thread.join()
        if self._own:
            self._signer.close()

    def __enter__(self) -> "SignatureService":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class Verifier:
    """Concurrent small verify calls behind shared launches (nwc_verifier): `verify` and
    `verify_batch` block like `Signature.verify` / `Signature.verify_batch` and raise CryptoError as
    they do, but calls made from several threads at once are packed into groups that share one
    launch.  A group closes at `max_requests` requests (0 = as many as fit), when it is full, or
    `max_wait_us` after its first request (0 = never wait for company).  A context manager;
    `close()` lets queued requests finish.  `lib`: a loaded library (tests)."""

    STATS = ("groups", "requests", "equations", "wide_equations", "cold_equations", "redone_equations",
             "bypassed_requests", "max_requests_in_group")

    def __init__(self, max_requests: int = 0, max_wait_us: int = 0, lib=None):
        self._lib = lib if lib is not None else _lib.load()
        self.handle = self._lib.nwc_verifier_create(max_requests, max_wait_us)
        if not self.handle:
            raise DeviceError("nwc_verifier_create failed (%d): %s" % (self._lib.nwc_last_error_code(),
                                                                       self._lib.nwc_last_error().decode()))

    def verify(self, digest, public_key, signature) -> None:
        """`Signature::verify` -> dalek verify_strict.  Raises CryptoError on an invalid signature."""
        d = digest.to_vec() if isinstance(digest, Digest) else bytes(digest)
        if len(d) != 32:
            raise ValueError("Digest must be 32 bytes")
        rc = _lib.check(self._lib.nwc_verifier_verify_strict(self.handle, _lib.buf(d), _lib.buf(bytes(public_key)),
                                                             _lib.buf(signature.flatten())))
        if rc != _lib.NWC_OK:
            raise CryptoError("signature verification failed")

    def verify_batch(self, digest, votes: Iterable[Tuple[PublicKey, "Signature"]], bad: Optional[list] = None) -> None:
        """`Signature::verify_batch(digest, votes)`.  Raises CryptoError if any vote fails; a list
        `bad` receives the indices of the failing votes."""
        d = digest.to_vec() if isinstance(digest, Digest) else bytes(digest)
        if len(d) != 32:
            raise ValueError("Digest must be 32 bytes")
        votes = list(votes)
        n = len(votes)
        pks = b"".join(bytes(p) for p, _ in votes)
        sigs = b"".join(s.flatten() for _, s in votes)
        bitmap = ctypes.create_string_buffer((n + 7) // 8 or 1)
        rc = _lib.check(self._lib.nwc_verifier_verify_batch(self.handle, _lib.buf(d), _lib.buf(pks) if n else None,
                                                            _lib.buf(sigs) if n else None, n, bitmap))
        if bad is not None:
            raw = bitmap.raw
            bad.extend(i for i in range(n) if (raw[i >> 3] >> (i & 7)) & 1)
        if rc != _lib.NWC_OK:
            raise CryptoError("batch verification failed")

    def stats(self) -> dict:
        out = (ctypes.c_uint64 * len(self.STATS))()
        _lib.check(self._lib.nwc_verifier_stats(self.handle, out))
        return {k: int(v) for k, v in zip(self.STATS, out)}

    def close(self) -> None:
        if self.handle:
            h, self.handle = self.handle, None
            _lib.check(self._lib.nwc_verifier_destroy(h))

    def __enter__(self) -> "Verifier":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter teardown)
            pass
