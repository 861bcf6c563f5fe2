"""strique_amd/csrc/vit_model.h -- the table of Viterbi kernel shapes, the decode modes each has and the functions that choose a
shape for a model, plain C++ -- under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/vit_shapes_check.cpp is compiled
as a stand-alone program (its own main, nothing loaded into Python) and run."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_vit_shapes_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "vit_shapes_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "vit_shapes_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"vit_shapes ok" in out.stdout, out.stdout.decode(errors="replace")
