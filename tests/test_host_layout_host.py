"""csrc/host_layout.hpp is plain C++17 with no HIP include: tests/host/host_layout_check.cpp, which includes nothing else
of the project, builds with the host compiler alone and its checks of Carve, the round-up and the two predicates hold."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host", "host_layout_check.cpp")


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


def test_host_layout_header_builds_and_checks_alone(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "host_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SOURCE], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "host_layout_check: ok" in run.stdout
