"""View requests in the sanitizer's group queue (narwhal_amd/csrc/sanitize_queue.h) on the CPU, under
the host sanitizers.

tests/cpp/sanitize_view_queue_host.cpp is a stand-alone program that drives the queue against a fake
backend (code = msg[0], kind = msg[1], a fake record, body length and body that are functions of the
message; a device thread with a random completion delay, one launch that fails, some slots marked
redo, left unwritten or left with the view flag unwritten): 8 threads x 2,000 requests, half of them
asking for a view, a quarter also for a vote, at max_messages=16 / max_wait_us=0 and at
max_messages=0 / max_wait_us=150.  It checks that a view comes back iff it was asked for and is the
caller's own; that a slot that did not ask never shows the device a non-zero wanted byte, also when
its buffer held a viewing group before; that redo words, unwritten words, unwritten flags and
oversized messages reach view_alone exactly once each, and that redo / bypass is not called as well
for such a request; that a failed launch gives its callers the error and a zeroed record; and that
stop() with viewers blocked returns.  It is built twice with g++, the sanitizer runtimes linked into
the program itself, and each binary runs as a child process; nothing is preloaded for it.
"""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "sanitize_view_queue_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def _build_and_run(name, sanitize):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread"] + sanitize +
                   ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "narwhal_amd", "csrc"),
                    "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _check(out):
    assert "stress max_messages=16 max_wait_us=0" in out
    assert "stress max_messages=0 max_wait_us=150" in out


def test_view_queue_under_thread_sanitizer():
    _check(_build_and_run("sanitize_view_queue_tsan", ["-fsanitize=thread", "-static-libtsan"]))


def test_view_queue_under_address_and_ub_sanitizers():
    _check(_build_and_run("sanitize_view_queue_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                       "-static-libasan", "-static-libubsan"]))
