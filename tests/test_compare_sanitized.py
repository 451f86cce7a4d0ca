"""csrc/bt_compare.hpp under AddressSanitizer and UndefinedBehaviorSanitizer, on the host: tests/cpp/compare_check.cpp is a
stand-alone program with its own main (nothing of it is loaded into Python), built here with the host compiler (g++: with the
sanitizers' runtimes linked statically, so the program does not depend on the order in which shared libraries are loaded).  It
runs the whole stage over frames whose planes are heap blocks of exactly their size and checks that every clamped tap of every
16 x 16 tile lies inside the 26 x 26 stage at the entry the SSIM kernel reads."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_compare_host_loop_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "compare_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           *(["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) and "clang" not in cxx else []),
           os.path.join(ROOT, "tests", "cpp", "compare_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host toolchain has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
