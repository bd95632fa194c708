"""Every runtime call of csrc/gt2d/gt2d.hip's entry point goes to the stream the caller handed over, in ONE launch per call, and
its kernel is launched.  No device: tests/test_objgt_record_host.py's arrangement -- the source compiled host-only, linked with
tests/host/hip_recorder.cpp -- for the next source with a driver of its own (``build.NESTED_SOURCES``,
tests/host/gt2d_record_main.cpp): a step of five frames in two dicts with all three kinds of point, the joints alone without a
bank, a step of one row, nothing to do, and three refusals.  The argument block is value-initialised: two stack fills give the
same record."""
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_launch_sequences", os.path.join(HERE, "golden", "make_golden_launch_sequences.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

SOURCE = "gt2d/gt2d.hip"
SENTINEL = ["--stream", "0x5eed00"]
KERNELS = {"gt2d_batch_kernel"}


def test_the_source_lists_are_disjoint_and_complete():
    """every .hip file under csrc/, subdirectories included, is built into the library exactly once"""
    from handobjectconsist_amd import build

    assert SOURCE in build.NESTED_SOURCES and not set(build.NESTED_SOURCES) & set(build.ALL_SOURCES)
    assert build.LIBRARY_SOURCES == build.ALL_SOURCES + build.NESTED_SOURCES
    on_disk = sorted(os.path.relpath(os.path.join(d, f), build.CSRC) for d, _, files in os.walk(build.CSRC) for f in files if f.endswith(".hip"))
    assert sorted(build.LIBRARY_SOURCES) == on_disk, "a source the library is not built from, or one that is missing"
    assert all(os.sep in src for src in build.NESTED_SOURCES)


@pytest.fixture(scope="module")
def driver():
    """(executable, kernel argument table): the host-only object and the device assembly's argument sizes of the one source, the
    driver and the recorder; cached under tests/host/build/ by content"""
    from handobjectconsist_amd import build

    os.makedirs(gen.CACHE, exist_ok=True)
    h = hashlib.sha256(" ".join(build.COMPILE_FLAGS).encode())
    files = [os.path.join(build.CSRC, f) for f in sorted(os.listdir(build.CSRC)) if f.endswith((".hpp", ".h"))] + [os.path.join(build.CSRC, SOURCE)]
    files += [os.path.join(gen.ROOT, "include", "meshraster_hip.h"), os.path.join(gen.HOST, "gt2d_record_main.cpp"), os.path.join(gen.HOST, "hip_recorder.cpp")]
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    stem = os.path.join(gen.CACHE, "gt2d_record.%s" % h.hexdigest()[:16])
    exe, table, obj = stem, stem + ".args.txt", stem + ".host.o"
    if os.path.exists(exe) and os.path.exists(table):
        return exe, table
    tmp = ".%d.tmp" % os.getpid()
    src = os.path.join(build.CSRC, SOURCE)
    subprocess.run([build._hipcc()] + build.COMPILE_FLAGS + ["-I", build.CSRC, "--cuda-host-only", "-c", "-o", obj, src], check=True, capture_output=True)
    asm = stem + tmp + ".s"
    subprocess.run([build._hipcc()] + build.COMPILE_FLAGS + ["-I", build.CSRC, "--cuda-device-only", "-S", "-o", asm, src], check=True, capture_output=True)
    with open(asm) as fh:
        kernels = gen.parse_kernel_args(fh.read())
    os.remove(asm)
    with open(table + tmp, "w") as fh:
        for name in sorted(kernels):
            fh.write("%s %d %s\n" % (name, len(kernels[name]), " ".join(map(str, kernels[name]))))
    os.replace(table + tmp, table)
    nm = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", nm)))
    cmd = [os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(gen.ROOT, "include"), "-o", exe + tmp,
           os.path.join(gen.HOST, "gt2d_record_main.cpp"), os.path.join(gen.HOST, "hip_recorder.cpp"), obj] + ["-Wl,--defsym=%s=0" % s for s in fatbins]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    os.replace(exe + tmp, exe)
    return exe, table


def launched(lines):
    return [l.split()[1] for l in lines if l.startswith("L ")]


def test_every_call_is_on_the_callers_stream_in_one_launch(driver):
    plain = gen.run_driver(*driver)
    on_stream = gen.run_driver(*driver, SENTINEL)
    assert on_stream == plain, "the stream changes a decision"
    off = [(name, l) for name, lines in on_stream.items() for l in lines if l.startswith("X ")]
    assert not off, "calls off the caller's stream: %s" % off
    assert not on_stream["never launched"], on_stream["never launched"]
    # one workgroup per 256 rows of all kinds together: 3 x 1031 + 2 x 65 object rows, 5 x 778 hand rows, 5 x 21 joints
    rows = 3 * 1031 + 2 * 65 + 5 * 778 + 5 * 21
    for name, blocks in (("gt2d_batch B5 three kinds", -(-rows // 256)), ("gt2d_batch B5 joints", 1), ("gt2d_batch one row", 1)):
        lines = [l for l in plain[name] if l.startswith("L ")]
        assert len(lines) == 1 and "gt2d_batch_kernel" in lines[0].split()[1], (name, plain[name])
        assert lines[0].split()[2:5] == ["%d,1,1" % blocks, "256", "0"], lines[0]
        assert plain[name][-1] == "R 0"
    assert -(-rows // 256) == 29
    assert {k for name in plain for k in KERNELS if any(k in l for l in launched(plain[name]))} == KERNELS
    for name, lines in plain.items():  # no memset, no allocation, no attribute anywhere
        assert not [l for l in lines if l[:2] in ("M ", "A ", "F ", "S ")], name


def test_nothing_to_do_and_refusals_launch_nothing(driver):
    cases = gen.run_driver(*driver, SENTINEL)
    for name, rc in (("gt2d_batch B0", 0), ("gt2d_batch no rows", 0), ("gt2d_batch short capacity", -1), ("gt2d_batch B0 with rows", -1),
                     ("gt2d_batch bank without vertices", -1)):
        assert cases[name] == ["R %d" % rc], (name, cases[name])


def test_the_record_does_not_depend_on_the_stack(driver):
    a = gen.run_driver(*driver, SENTINEL + ["--stack-fill", "0"])
    b = gen.run_driver(*driver, SENTINEL + ["--stack-fill", "165"])
    assert a == b
