#!/usr/bin/env python3
"""Writes tests/golden/vote_sigs.json: 257 (id, round, origin) triples and the signatures
Vote::new gives them under one seed, from the pure-Python restatement
(oracle/ed25519_ref.py sign(seed, digest72(id, round, origin)), digest72 of oracle/messages_ref.py).
The restatement takes ~0.2 s per signature, so tests/test_gpu_vote.py reads this file and signs
only a sample again.  Ids and origins are hash output (not necessarily points: a vote only hashes
them); the rounds begin with the values at which the two u32 halves of the round can be swapped or
dropped.  Deterministic: running it again writes the same file.

    python tools/gen_vote_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ed25519_ref as ed  # noqa: E402
import messages_ref as mr  # noqa: E402

N = 257
EDGE_ROUNDS = [1 << 32, (1 << 64) - 1, (1 << 32) - 1, 0, 1]


def stream(tag: bytes, i: int) -> bytes:
    return hashlib.sha512(b"narwhal-amd vote golden " + tag + i.to_bytes(8, "little")).digest()


def triples():
    out = []
    for i in range(N):
        rnd = EDGE_ROUNDS[i] if i < len(EDGE_ROUNDS) else int.from_bytes(stream(b"round", i)[:8], "little")
        out.append((stream(b"id", i)[:32], rnd, stream(b"origin", i)[:32]))
    return out


def main():
    seed = stream(b"seed", 0)[:32]
    cases = [{"id": i.hex(), "round": r, "origin": o.hex(), "sig": ed.sign(seed, mr.digest72(i, r, o)).hex()}
             for i, r, o in triples()]
    path = os.path.join(ROOT, "tests", "golden", "vote_sigs.json")
    with open(path, "w") as f:
        json.dump({"seed": seed.hex(), "public_key": ed.public_key(seed).hex(), "cases": cases}, f, indent=0)
        f.write("\n")
    print(path, len(cases))


if __name__ == "__main__":
    main()
