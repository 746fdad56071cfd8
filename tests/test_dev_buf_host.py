"""Device buffer ownership (narwhal_amd/csrc/dev_buf.h) on the CPU, under the host sanitizers.

tests/cpp/dev_buf_host.cpp is a stand-alone program that drives Buf and BufSet with a counting fake
allocator: every block freed exactly once and by a call of the right kind, release and alloc over a
held block, failed frees, bytes(account) against the requested sizes at every step,
release_trimmable, the allocation sequences of ensure_verify_tables and auto_grow with each of
their allocations failing in turn, and ensure against worked values of the two growth policies.
It is built with g++, the sanitizer runtimes linked into the program itself, and runs as a child
process; nothing is preloaded for it.
"""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "dev_buf_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
HEADER = os.path.join(ROOT, "narwhal_amd", "csrc", "dev_buf.h")


def test_dev_buf_under_address_and_ub_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "dev_buf_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "narwhal_amd", "csrc"), "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    assert lines[:-1] == ["release", "accounts", "trim", "tables retry", "auto_grow retry", "ensure"]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_dev_buf_header_has_no_hip():
    text = open(HEADER).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for word in ("hip/", "hipStream", "hipError", "hipEvent", "hipMalloc", "hipFree", "hipHost", "__global__", "__device__"):
        assert word not in code, word
