"""The message pipeline's host decisions (narwhal_amd/csrc/msg_plan.h) on the CPU, under the host sanitizers.

tests/cpp/msg_plan_host.cpp is a stand-alone program that checks message_cuts against worked values
and its post-condition (first cut 0, last cut m, strictly increasing, every interior cut a multiple
of 64) over a sweep of batch shapes and chunk sizes, vote_slots and its limit, the call arena's and
the message arena's layouts (alignment, order, no overlap, total size against the sizes written out
in the test), the pinned stage's layout at the chunk limit, and schedule's truth table.  It is built
with g++, the sanitizer runtimes linked into the program itself, and runs as a child process;
nothing is preloaded for it.
"""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "msg_plan_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
HEADER = os.path.join(ROOT, "narwhal_amd", "csrc", "msg_plan.h")


def test_msg_plan_under_address_and_ub_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "msg_plan_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "narwhal_amd", "csrc"),
                    "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    assert lines[:-1] == ["message_cuts worked", "message_cuts sweep", "vote_slots", "layouts", "pinned stage", "schedule"]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_msg_plan_header_has_no_hip():
    text = open(HEADER).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for word in ("hip/", "hipStream", "hipError", "hipEvent", "__global__", "__device__"):
        assert word not in code, word
