"""Child process of tests/test_gpu_vote.py (libnwc reads its environment once per process, and
nwc_shutdown ends a process's use of the device):

  bypass        NWC_SANITIZER_GROUP_BYTES=4096 in the environment: a header of 200 parents is larger
                than a group and is handed to the batch entry; its vote comes from the one-message route
  wrong_device  NWC_VIRTUAL_DEVICES=2: a signer on context 1, a sanitizer on context 0
  shutdown      nwc_shutdown with a live sanitizer and signer, then sanitize_vote

usage: vote_helper.py MODE ROOT; prints one JSON line."""
import json
import os
import sys

mode, root = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "oracle"))

import ed25519_ref as ed  # noqa: E402
from narwhal_amd import _lib  # noqa: E402
from tests.oracle_lib import load_oracle  # noqa: E402
from tests.test_gpu_sanitizer import _World  # noqa: E402
from tests.test_gpu_vote import SV, make_signer  # noqa: E402

lib = _lib.load()
w = _World(load_oracle(), 4, 21)
seed = w.rand32()
out = {}
if mode == "bypass":
    w.install(lib)
    signer = make_signer(lib, w.o, seed)
    hdr, hid = w.header(2, 9, 200)
    msg = w.mr.msg_header(hdr)
    with SV(lib, 0, 0) as s:
        rc, dig, kind, sig, voted = s.vote(signer, msg)
        exp = w.expect(msg)
        out["len"] = len(msg)
        out["ok"] = rc == exp[0] == 0 and dig == exp[2] == hid and kind == 0
        out["voted"] = voted
        out["sig_ok"] = sig == ed.sign(seed, w.mr.digest72(hid, 9, w.pks[2]))
        out["stats"] = s.stats()
        out["vote_stats"] = s.vote_stats()
    out["destroy"] = lib.nwc_signer_destroy(signer)
elif mode == "wrong_device":
    out["devices"] = lib.nwc_device_count()
    _lib.check(lib.nwc_dev_set_device(1))
    signer1 = make_signer(lib, w.o, seed)
    _lib.check(lib.nwc_dev_set_device(0))
    w.install(lib)
    signer0 = make_signer(lib, w.o, seed)
    hdr, hid = w.header(1, 3, 2)
    msg = w.mr.msg_header(hdr)
    with SV(lib, 0, 0) as s:
        rc, dig, kind, sig, voted = s.vote(signer1, msg)
        out["rc"] = rc
        out["code"] = lib.nwc_last_error_code()
        out["voted"] = voted
        out["sig_zero"] = sig == bytes(64)
        out["stats_after_refusal"] = s.stats()
        rc, dig, kind, sig, voted = s.vote(signer0, msg)   # the same call with a signer of this device
        out["same_device"] = [rc, voted, sig == ed.sign(seed, w.mr.digest72(hid, 3, w.pks[1]))]
    out["destroy"] = [lib.nwc_signer_destroy(signer0), lib.nwc_signer_destroy(signer1)]
elif mode == "shutdown":
    w.install(lib)
    signer = make_signer(lib, w.o, seed)
    hdr, hid = w.header(0, 3, 2)
    msg = w.mr.msg_header(hdr)
    s = SV(lib, 0, 0)
    rc, dig, kind, sig, voted = s.vote(signer, msg)
    out["before"] = [rc, voted]
    lib.nwc_shutdown()
    rc, dig, kind, sig, voted = s.vote(signer, msg)
    out["after_shutdown"] = [rc, voted, sig == bytes(64)]
    out["destroy"] = [lib.nwc_sanitizer_destroy(s.h), lib.nwc_signer_destroy(signer)]
    s.h = None
print(json.dumps(out))
