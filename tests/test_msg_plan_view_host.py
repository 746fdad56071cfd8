"""The call arena of nwc_sanitize_messages_view (narwhal_amd/csrc/msg_plan.h) on the CPU, under
the host sanitizers.

tests/cpp/msg_plan_view_host.cpp is a stand-alone program: the call arena with the view records,
the body and its counter at m = 1, 63, 64, 65 and 4,097 (every field aligned, sized for its array,
none overlapping, the total against the sizes written out in the test), the body bound, and that a
call without views keeps today's offsets for all four (own_state, votes) combinations.  It is built
with g++, the sanitizer runtimes linked into the program itself, and runs as a child process;
nothing is preloaded for it.
"""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "msg_plan_view_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def test_msg_plan_view_under_address_and_ub_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "msg_plan_view_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "narwhal_amd", "csrc"),
                    "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert lines == ["body bound", "call arena", "ok"], r.stdout[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
