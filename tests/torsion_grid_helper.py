"""Subprocess body of tests/test_gpu_torsion_grid.py's two child tests: libnwc reads
NWC_VERIFY_MAX_LAUNCH and NWC_VIRTUAL_DEVICES once, in nwc_init, so each runs in a process of its own.

    torsion_grid_helper.py launches in.npz out.npz ROOT    the device entry, once per seed
    torsion_grid_helper.py devices  in.npz out.npz ROOT    the host entry with the committee set

Writes the certificate and bad-vote bitmaps per seed (the parent compares them with the oracle)."""
import ctypes
import sys

import numpy as np

mode, src, dst, root = sys.argv[1:5]
sys.path.insert(0, root)
import torch  # noqa: E402,F401
from narwhal_amd import _lib, device  # noqa: E402

lib = _lib.load()
d = dict(np.load(src))
dig, offs, pks, sigs = (np.ascontiguousarray(d[k]) for k in ("dig", "offs", "pks", "sigs"))
m, nv = len(offs) - 1, int(offs[-1])
out = {"devices": np.array([lib.nwc_device_count()]), "cert": [], "bad": []}
try:
    if mode == "devices":
        cm = np.ascontiguousarray(d["committee"])
        _lib.check(lib.nwc_set_committee(_lib.buf(cm), len(cm)))
        cuts = np.zeros(lib.nwc_device_count() + 1, np.uint64)
        _lib.check(lib.nwc_cert_cuts(_lib.buf(offs.astype(np.uint32)), m, lib.nwc_device_count(), _lib.buf(cuts)))
        out["cuts"] = cuts.astype(np.int64)
    for seed in d["seeds"]:
        _lib.diag_set("dalek_seed", int(seed))
        if mode == "devices":
            cert = ctypes.create_string_buffer((m + 7) // 8)
            bad = ctypes.create_string_buffer((nv + 7) // 8)
            _lib.check(lib.nwc_verify_batch_msm_many(_lib.buf(dig), _lib.buf(offs.astype(np.uint32)), _lib.buf(pks),
                                                     _lib.buf(sigs), m, cert, bad))
            out["cert"].append(np.frombuffer(cert.raw, np.uint8).copy())
            out["bad"].append(np.frombuffer(bad.raw, np.uint8).copy())
        else:
            assert mode == "launches"
            t = lambda a, dt=torch.uint8: torch.from_numpy(a).to(dt).cuda()  # noqa: E731
            do = t(offs.astype(np.int32), torch.int32)
            mi = np.repeat(np.arange(m, dtype=np.int32), np.diff(offs))
            leaf = device.verify_batch_msm(t(dig), do, t(mi, torch.int32), t(pks), t(sigs))
            cert, bad = device.cert_reduce(leaf, do, nv)
            torch.cuda.synchronize()
            out["cert"].append(np.packbits(device.unpack_bits(cert, m), bitorder="little"))
            out["bad"].append(np.packbits(device.unpack_bits(bad, nv), bitorder="little"))
finally:
    _lib.diag_set("dalek_seed", 0)
    if mode == "devices":
        _lib.check(lib.nwc_set_committee(None, 0))
out["cert"], out["bad"] = np.stack(out["cert"]), np.stack(out["bad"])
np.savez(dst, **out)
