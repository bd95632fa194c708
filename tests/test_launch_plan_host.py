"""csrc/launch_plan.hpp is plain C++17 with no HIP include: tests/host/launch_plan_check.cpp builds with the host compiler alone
and asserts the invariants the kernels rely on -- LDS within the limit, grids within 2^31 - 1, parts a power of two within the
workspace's, a box buffer that holds the largest part, two launches exactly from eight parts on, the scatter's table and
workgroups per image, the fused strip-gather only with list and strips -- over an exhaustive small grid plus the benchmark shapes."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host", "launch_plan_check.cpp")


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


def test_launch_plans_keep_the_kernels_invariants(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "launch_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SOURCE], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "launch_plan_check: ok" in run.stdout
