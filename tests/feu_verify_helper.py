"""Subprocess helper for tests/test_gpu_feu.py: verifies prefixes of the triples in an .npz through
the device entry (strict and leaf) and writes the verdicts.  The route comes from the environment
(NWC_COLD, NWC_FORCE_FALLBACK_EVERY), which libnwc reads once per process."""
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[3])
from narwhal_amd import device  # noqa: E402

d = np.load(sys.argv[1])
m, p, s = (torch.from_numpy(d[k]).cuda() for k in ("m", "p", "s"))
out = {}
for n in (int(x) for x in sys.argv[4].split(",")):
    for strict in (True, False):
        w = device.verify(m[:n].contiguous(), p[:n].contiguous(), s[:n].contiguous(), strict=strict)
        torch.cuda.synchronize()
        out["%s%d" % ("s" if strict else "l", n)] = device.unpack_bits(w, n)
np.savez(sys.argv[2], **out)
