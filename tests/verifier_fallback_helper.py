"""Child process of tests/test_gpu_verifier.py::test_redo_path.  The parent sets
NWC_FORCE_FALLBACK_EVERY=3 (read once per process), so every third first-sight equation of a
group answers "decide me again" and is redone on the general path.  200 mixed requests -- strict
single votes and certificates of 1 to 40 votes, a fifth corrupted -- go through one verifier from 8
threads; the last line printed is a JSON object with the verifier's stats and the number of
answers that differ from the CPU oracle."""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.oracle_lib import load_oracle  # noqa: E402
from tests.test_gpu_verifier import V, _random_requests  # noqa: E402


def main():
    from narwhal_amd import _lib
    assert os.environ.get("NWC_FORCE_FALLBACK_EVERY") == "3"
    lib = _lib.load()
    oracle = load_oracle()
    reqs = _random_requests(oracle, 61, 200, 40)
    with V(lib, 0, 0) as v, ThreadPoolExecutor(8) as pool:
        def run(r):
            strict, digest, pks, sigs = r
            if strict:
                ok = v.strict(digest, pks[0], sigs[0])
                return ok, np.array([ok])
            return v.batch(digest, pks, sigs)
        got = list(pool.map(run, reqs))
        stats = v.stats()
    mismatches = invalid = 0
    for (strict, digest, pks, sigs), (ok, valid) in zip(reqs, got):
        tiled = np.tile(digest, (pks.shape[0], 1))
        exp = oracle.strict_many(tiled, pks, sigs) if strict else oracle.leaf_many(tiled, pks, sigs)
        mismatches += int(not (valid == exp).all() or ok != bool(exp.all()))
        invalid += not ok
    print(json.dumps({"requests": len(reqs), "mismatches": mismatches, "invalid": int(invalid), "stats": stats,
                      "strict_requests": sum(r[0] for r in reqs), "batch_requests": sum(not r[0] for r in reqs)}))


if __name__ == "__main__":
    main()
