#!/usr/bin/env python3
"""Generates tests/golden/torsion_grid.json: one vote for every cell (a, b) of E[8] x E[8], the
inputs that span dalek's batch equation as narwhal_amd/csrc/resolve.h evaluates it in Z/8.

    python tests/golden/make_torsion_grid.py

With G8 = ed25519_ref.G8_HEX (a generator of the 8-torsion group) and T[j] = [j] G8:

  * key b (b = 0..7) is A_b = sec_b B + T[5b mod 8], so l A_b = [b] G8 (l = 5 mod 8, 25 = 1 mod 8);
  * vote (a, b) is signed by A_b over the one 32-byte message `msg` with R = r B + T[c] and
    s = r + k sec_b mod l, k = H(R || A_b || msg): its residual is
        e = s B - R - k A_b = -T[c] - k T[5b] = [(-c - 5 b k) mod 8] G8,
    and (r, c) are searched until that is [a] G8.

Cell (0, 0) is an honest vote; the other 63 are in dalek's randomized class (the verdict of a batch
holding them depends on the z_i).  Each key signs eight distinct votes over the same message, which is
what the repeated-key cases of the Pippenger groups need.  Everything is derived from SHA-512 of fixed
labels, so the file is reproducible; only oracle/ed25519_ref.py is used (pure Python, ~10 s).
tests/test_torsion_grid_host.py re-derives every label from the stored bytes.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ed25519_ref as o  # noqa: E402

OUT = os.path.join(HERE, "torsion_grid.json")
FILLERS = 12


def _scalar(label: str) -> int:
    return o.scalar_from_hash(o.sha512(b"narwhal-amd torsion grid: " + label.encode()))


def main() -> None:
    g8 = o.decompress(bytes.fromhex(o.G8_HEX))
    T = [o.pt_mul(j, g8) for j in range(8)]
    msg = o.sha512(b"narwhal-amd torsion grid: msg")[:32]
    keys, votes, trials_max = [], [], 0
    for b in range(8):
        sec = _scalar("key %d" % b)
        tb = 5 * b % 8
        A = o.pt_add(o.pt_mul(sec, o.BASEPOINT), T[tb])
        pk = o.compress(A)
        keys.append(pk.hex())
        for a in range(8):
            found, trial = None, 0
            while found is None:
                r = _scalar("vote %d %d trial %d" % (a, b, trial))
                trial += 1
                rB = o.pt_mul(r, o.BASEPOINT)
                for c in range(8):
                    Rb = o.compress(o.pt_add(rB, T[c]))
                    k = o.scalar_from_hash(o.sha512(Rb + pk + msg))
                    if (-c - k * tb) % 8 == a:
                        s = (r + k * sec) % o.L
                        found = Rb + s.to_bytes(32, "little")
                        break
            trials_max = max(trials_max, trial)
            votes.append({"a": a, "b": b, "pk": pk.hex(), "sig": found.hex()})
    doc = {
        "about": "E[8] x E[8] torsion grid (tests/golden/make_torsion_grid.py): vote (a, b) has residual "
                 "e = [a] G8 and a key with l A = [b] G8; G8 = " + o.G8_HEX,
        "msg": msg.hex(),
        "keys": keys,
        "votes": votes,
        "filler_seeds": [o.sha512(b"narwhal-amd torsion grid: filler %d" % i)[:32].hex() for i in range(FILLERS)],
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s: %d votes, at most %d trials per cell" % (os.path.relpath(OUT, ROOT), len(votes), trials_max))


if __name__ == "__main__":
    main()
