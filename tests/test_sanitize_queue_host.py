"""The sanitizer's group queue (narwhal_amd/csrc/sanitize_queue.h) on the CPU, under the host sanitizers.

tests/cpp/sanitize_queue_host.cpp is a stand-alone program that drives the queue against a fake
backend (code = msg[0], a device thread with a random completion delay, one launch that fails, some
slots marked redo or left unwritten): 8 threads x 2,000 requests of 1 to 20,000 bytes.  It checks
that every caller gets exactly its own code, digest and kind, that no group exceeds max_messages or
the byte capacity, that every range starts 16-byte aligned and no two overlap, that every request
is answered exactly once, that the failed group's callers and only they get the error code, that
redo and unwritten words go through the backend's redo call, that oversized requests go through
bypass, and that stop() with callers blocked returns after they have left.  It is built twice with
g++, the sanitizer runtimes linked into the program itself, and each binary runs as a child
process; nothing is preloaded for it.
"""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "sanitize_queue_host.cpp")
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


def test_queue_under_thread_sanitizer():
    out = _build_and_run("sanitize_queue_tsan", ["-fsanitize=thread", "-static-libtsan"])
    assert "stress max_messages=16 max_wait_us=0" in out


def test_queue_under_address_and_ub_sanitizers():
    out = _build_and_run("sanitize_queue_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                 "-static-libasan", "-static-libubsan"])
    assert "stress max_messages=0 max_wait_us=150" in out


def test_queue_header_has_no_hip():
    text = open(os.path.join(ROOT, "narwhal_amd", "csrc", "sanitize_queue.h")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for word in ("hip/", "hipStream", "hipError", "__global__", "__device__"):
        assert word not in code, word
