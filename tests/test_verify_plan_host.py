"""The host verify path's decisions (narwhal_amd/csrc/verify_plan.h) on the CPU, under the host sanitizers.

tests/cpp/verify_plan_host.cpp is a stand-alone program that checks Settings::parse against fake
environments (every default of README's table, each rounding and clamp, what switches a switch
off), chunk_cuts against worked values and its properties over a sweep of sizes, route_verify
against a hand-written table of the launches launch_verify's comments name and against its
invariants over every combination of the device view's facts, small_call_route, and poll_written
with and without a writer.  It is built with g++, the sanitizer runtimes linked into the program
itself, and runs as a child process; nothing is preloaded for it.
"""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "verify_plan_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
HEADER = os.path.join(ROOT, "narwhal_amd", "csrc", "verify_plan.h")


def test_plan_under_address_and_ub_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "verify_plan_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "narwhal_amd", "csrc"),
                    "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    assert lines[:-1] == ["settings", "chunk_cuts", "route table", "route invariants", "small_call_route", "poll_written"]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_plan_header_has_no_hip():
    text = open(HEADER).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for word in ("hip/", "hipStream", "hipError", "hipEvent", "__global__", "__device__"):
        assert word not in code, word
