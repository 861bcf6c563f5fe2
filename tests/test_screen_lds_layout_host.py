"""strique_amd/csrc/screen_lds_layout.h -- the lane-major LDS image of the two-flank screen's score tables: slot of a lane, row bases,
the address of (lane, class, level), the bytes needed and the limit above which a launch falls back to the class rows, plain C++ --
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/screen_lds_layout_check.cpp is compiled as a stand-alone program
(its own main, nothing loaded into Python) and run."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_screen_lds_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "screen_lds_layout_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "screen_lds_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"screen_lds_layout ok" in out.stdout, out.stdout.decode(errors="replace")
