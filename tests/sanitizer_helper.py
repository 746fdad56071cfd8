"""Child process of tests/test_gpu_sanitizer.py (libnwc reads its environment once per process, and
nwc_shutdown ends a process's use of the device):

  bypass    NWC_SANITIZER_GROUP_BYTES=4096 in the environment: a certificate of ~10 KB is handed to
            nwc_sanitize_messages, a vote in the same sanitizer is grouped; both against the restatement
  shutdown  nwc_shutdown with a live sanitizer: it answers NWC_ERR_NOT_INIT from then on, also after
            the library was initialised again, and is destroyed all the same

usage: sanitizer_helper.py MODE ROOT; prints one JSON line."""
import json
import os
import sys

mode, root = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "oracle"))

from narwhal_amd import _lib  # noqa: E402
from tests.oracle_lib import load_oracle  # noqa: E402
from tests.test_gpu_sanitizer import S, _World  # noqa: E402

lib = _lib.load()
w = _World(load_oracle(), 66, 7)
w.install(lib)
vote = w.vote(3, w.rand32(), 4, w.pks[5])
out = {}
if mode == "bypass":
    cert = w.certificate(2, 6, list(range(66)), nparents=66)
    with S(lib, 0, 0) as s:
        got = s(cert)
        exp = w.expect(cert)
        out["cert_len"] = len(cert)
        out["cert_ok"] = got[0] == exp[0] == 0 and got[1] == exp[2] and got[2] == 2
        out["after_cert"] = s.stats()
        got = s(vote)
        exp = w.expect(vote)
        out["vote_ok"] = got[0] == exp[0] == 0 and got[1] == exp[2] and got[2] == 1
        out["after_vote"] = s.stats()
elif mode == "shutdown":
    s = S(lib, 0, 0)
    out["before"] = s.raw(vote)[0]
    lib.nwc_shutdown()
    out["after_shutdown"] = s.raw(vote)[0]
    _lib.check(lib.nwc_init(0))
    out["after_reinit"] = s.raw(vote)[0]
    out["destroy"] = lib.nwc_sanitizer_destroy(s.h)
    s.h = None
print(json.dumps(out))
