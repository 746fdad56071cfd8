"""Subprocess body of tests/test_gpu_memory.py::test_trim_walk_in_a_fresh_process: a fresh process
without a committee runs five verification calls over GPU-signed votes of 16 keys (every 7th
corrupted), nwc_trim, and the five calls again, and writes nwc_memory_info after every step
(argv[1]: the JSON file, argv[2]: the repository root).  Every verdict is checked against the
construction here; the test compares the memory figures."""
import ctypes
import json
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[2])
from narwhal_amd import _lib, device  # noqa: E402

FIELDS = ("tables", "committee", "auto_cache", "scratch")
N_STRICT, N_LEAF, M, Q = 4096, 65536, 64, 8   # N_LEAF: the launch-key threshold (launch_keys.h)
NV = M * Q

lib = _lib.load()
steps = []


def note(name):
    torch.cuda.synchronize()
    mem = _lib.memory_info()
    steps.append(dict(step=name, **{k: int(mem[k]) for k in FIELDS}))


note("start")
seeds = device.derive32(b"walk-seed", 0, 16)
who = torch.arange(N_LEAF, device="cuda") % 16
msgs = device.derive32(b"walk-msg", 0, N_LEAF)
pks, sigs = device.keygen_sign(seeds[who], msgs)
sigs[::7, 40] ^= 1
cdig = device.derive32(b"walk-cert", 0, M)
mi = torch.arange(M, device="cuda", dtype=torch.int32).repeat_interleave(Q)
cpks, csigs = device.keygen_sign(seeds[who[:NV]], cdig[mi.long()].contiguous())
csigs[::7, 40] ^= 1
offs = torch.arange(M + 1, device="cuda", dtype=torch.int32) * Q
valid = np.arange(N_LEAF) % 7 != 0                 # equation i of either set is valid iff i % 7 != 0
cert_ok = valid[:NV].reshape(M, Q).all(axis=1)
host = [np.ascontiguousarray(t.cpu().numpy()) for t in (cdig, cpks, csigs)]
offs_host = offs.cpu().numpy().astype(np.uint32)
note("inputs")


def five_calls(tag):
    got = device.unpack_bits(device.verify(msgs[:N_STRICT], pks[:N_STRICT], sigs[:N_STRICT], strict=True), N_STRICT)
    assert (got == valid[:N_STRICT]).all(), tag + "strict"
    note(tag + "strict")
    got = device.unpack_bits(device.verify(msgs, pks, sigs, strict=False), N_LEAF)
    assert (got == valid).all(), tag + "leaf"
    note(tag + "leaf")
    for name, f in (("straus", device.verify_batch_straus), ("msm", device.verify_batch_msm)):
        cw, bw = device.cert_reduce(f(cdig, offs, mi, cpks, csigs), offs, NV)
        assert (device.unpack_bits(bw, NV) == ~valid[:NV]).all() and (device.unpack_bits(cw, M) == cert_ok).all(), tag + name
        note(tag + name)
    cert = ctypes.create_string_buffer((M + 7) // 8)
    bad = ctypes.create_string_buffer((NV + 7) // 8)
    _lib.check(lib.nwc_verify_batch_msm_many(_lib.buf(host[0]), _lib.buf(offs_host), _lib.buf(host[1]), _lib.buf(host[2]), M,
                                             cert, bad))
    c = np.unpackbits(np.frombuffer(cert.raw, np.uint8), bitorder="little")[:M].astype(bool)
    b = np.unpackbits(np.frombuffer(bad.raw, np.uint8), bitorder="little")[:NV].astype(bool)
    assert (c == cert_ok).all() and (b == ~valid[:NV]).all(), tag + "dalek"
    note(tag + "dalek")


five_calls("1:")
_lib.check(lib.nwc_trim())
note("trim")
five_calls("2:")
json.dump({"build_id": lib.nwc_build_id().decode(), "steps": steps}, open(sys.argv[1], "w"), indent=1)
