"""strique_amd/csrc/detect_plan.h -- the host-side bookkeeping of the detect pipeline, plain C++ -- under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host/detect_plan_check.cpp is compiled as a stand-alone program (its own main, nothing loaded
into Python) and run."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_detect_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "detect_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "detect_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"detect_plan ok" in out.stdout, out.stdout.decode(errors="replace")
