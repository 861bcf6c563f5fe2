"""strique_amd/csrc/screen_levels_layout.h -- the level image of the coarse two-flank screen's score tables: the address of (lane, class,
level), the pre-evaluated band clamp, the bytes needed, the limit above which a launch falls back to the lane-major image and the byte
scale, plain C++ -- under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/screen_levels_layout_check.cpp is compiled as a
stand-alone program (its own main, nothing loaded into Python) and run."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_screen_levels_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "screen_levels_layout_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "screen_levels_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"screen_levels_layout ok" in out.stdout, out.stdout.decode(errors="replace")
