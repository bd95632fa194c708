"""Every runtime call of csrc/obj_gt.hip's entry points goes to the stream the caller handed over, and both of its kernels are
launched.  No device: tests/test_stream_record_host.py's arrangement -- the source compiled host-only, linked with
tests/host/hip_recorder.cpp -- for a source with a driver of its own (``build.OWN_DRIVER_SOURCES``,
tests/host/obj_gt_record_main.cpp): a bank of three models, a step of five frames in two dicts, no model, no frame, and two
refusals.  The argument blocks are value-initialised: two stack fills give the same record."""
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

SOURCE = "obj_gt.hip"
SENTINEL = ["--stream", "0x5eed00"]
KERNELS = {"obj_bank_build_kernel", "obj_gt_batch_kernel"}


def test_the_source_lists_are_disjoint_and_complete():
    from handobjectconsist_amd import build

    assert build.OWN_DRIVER_SOURCES == [SOURCE] and not set(build.OWN_DRIVER_SOURCES) & set(build.SOURCES)
    assert build.ALL_SOURCES == build.SOURCES + build.OWN_DRIVER_SOURCES
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(build.ALL_SOURCES) == on_disk, "a source the library is not built from, or one that is missing"


@pytest.fixture(scope="module")
def driver():
    """(executable, kernel argument table): the host-only object and the device assembly's argument sizes of the one source, the
    driver and the recorder; cached under tests/host/build/ by content"""
    from handobjectconsist_amd import build

    os.makedirs(gen.CACHE, exist_ok=True)
    h = hashlib.sha256(" ".join(build.COMPILE_FLAGS).encode())
    files = [os.path.join(build.CSRC, f) for f in sorted(os.listdir(build.CSRC)) if f.endswith((".hpp", ".h")) or f == SOURCE]
    files += [os.path.join(gen.ROOT, "include", "meshraster_hip.h"), os.path.join(gen.HOST, "obj_gt_record_main.cpp"), os.path.join(gen.HOST, "hip_recorder.cpp")]
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    stem = os.path.join(gen.CACHE, "obj_gt_record.%s" % h.hexdigest()[:16])
    exe, table, obj = stem, stem + ".args.txt", stem + ".host.o"
    if os.path.exists(exe) and os.path.exists(table):
        return exe, table
    tmp = ".%d.tmp" % os.getpid()
    src = os.path.join(build.CSRC, SOURCE)
    subprocess.run([build._hipcc()] + build.COMPILE_FLAGS + ["--cuda-host-only", "-c", "-o", obj, src], check=True, capture_output=True)
    asm = stem + tmp + ".s"
    subprocess.run([build._hipcc()] + build.COMPILE_FLAGS + ["--cuda-device-only", "-S", "-o", asm, src], check=True, capture_output=True)
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
           os.path.join(gen.HOST, "obj_gt_record_main.cpp"), os.path.join(gen.HOST, "hip_recorder.cpp"), obj] + ["-Wl,--defsym=%s=0" % s for s in fatbins]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    os.replace(exe + tmp, exe)
    return exe, table


def launched(lines):
    return [l.split()[1] for l in lines if l.startswith("L ")]


def test_every_call_is_on_the_callers_stream_and_every_kernel_is_launched(driver):
    plain = gen.run_driver(*driver)
    on_stream = gen.run_driver(*driver, SENTINEL)
    assert on_stream == plain, "the stream changes a decision"
    off = [(name, l) for name, lines in on_stream.items() for l in lines if l.startswith("X ")]
    assert not off, "calls off the caller's stream: %s" % off
    assert not on_stream["never launched"], on_stream["never launched"]
    build_l, batch_l = launched(plain["obj_bank_build models3"]), launched(plain["obj_gt_batch B5"])
    assert len(build_l) == 1 and "obj_bank_build_kernel" in build_l[0] and len(batch_l) == 1 and "obj_gt_batch_kernel" in batch_l[0]
    # one workgroup per model; one workgroup per 256 vertex rows (3 x 1031 + 2 x 65), per 256 face rows (3 x 2000 + 2 x 129) and per
    # 256 of the 4 x 5 centre / scale values
    line = [l for l in plain["obj_bank_build models3"] if l.startswith("L ")][0].split()
    assert line[2:5] == ["3,1,1", "256", "0"], line
    blocks = -(-(3 * 1031 + 2 * 65) // 256) + -(-(3 * 2000 + 2 * 129) // 256) + -(-(4 * 5) // 256)
    line = [l for l in plain["obj_gt_batch B5"] if l.startswith("L ")][0].split()
    assert blocks == 13 + 25 + 1 and line[2:5] == ["%d,1,1" % blocks, "256", "0"], line
    for name, lines in plain.items():  # no memset, no allocation, no attribute anywhere
        assert not [l for l in lines if l[:2] in ("M ", "A ", "F ", "S ")], name


def test_nothing_to_do_and_refusals_launch_nothing(driver):
    cases = gen.run_driver(*driver, SENTINEL)
    for name, rc in (("obj_bank_build models0", 0), ("obj_gt_batch B0", 0), ("obj_gt_batch B5 short capacity", -1), ("obj_gt_batch B0 with rows", -1)):
        assert cases[name] == ["R %d" % rc], (name, cases[name])
    assert cases["obj_bank_build models3"][-1] == "R 0" and cases["obj_gt_batch B5"][-1] == "R 0"


def test_the_record_does_not_depend_on_the_stack(driver):
    a = gen.run_driver(*driver, SENTINEL + ["--stack-fill", "0"])
    b = gen.run_driver(*driver, SENTINEL + ["--stack-fill", "165"])
    assert a == b
