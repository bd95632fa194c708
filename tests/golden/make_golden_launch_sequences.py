"""Generate tests/golden/launch_sequences.json: what every launcher of raster_fwd.hip, raster_bwd.hip, raster_bwd_vc.hip, warp.hip,
warp_tiles.hip, pair_step.hip and vertex_stage.hip asks of the HIP runtime -- kernel, grid, block, dynamic LDS bytes and a hash of the explicit arguments of
each launch, every memset, stream-ordered allocation and attribute call, in order -- over the table of cases in
tests/host/launch_record_main.cpp.  No device is involved: the seven sources are compiled with the library's flags plus
``--cuda-host-only`` and linked with tests/host/hip_recorder.cpp, a stand-in for the runtime that writes the calls down.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_launch_sequences.py [output path [source hash]]

The file is a record of the launchers as they were BEFORE their decisions moved into csrc/launch_plan.hpp, with one host-side
change on top.  Seven parameter blocks were list-initialised, which left their padding bytes -- kernel-argument bytes like any
other -- to the stack, so that the hashes of their launches differed from run to run or from build to build: PairParams and
PairBwdParams (warp.hip), the two PixelMapParams of mr_backward_pixel_map and mr_render_backward (raster_bwd.hip), and the
GatherVCParams of mr_render_vc_backward (inside its ScatterVCParams), mr_render_flow_backward, mr_flow_pair_backward_tiles_crit
and launch_unit_scatter_tiles (raster_bwd_vc.hip).  In the recorded tree they are value-initialised and then filled, exactly as in the
tree this file came with; nothing else differs from the parent commit, and against the untouched parent only the argument
hashes of those launches differ.  The ``build.source_hash()`` of the recorded tree is stored with the file.

The file is not regenerated from later code: a line that differs is a launch whose kernel, grid, LDS size or arguments changed.  When a decision is MEANT to change, record the file again from the commit
before the change, check that the test passes there, make the change, record once more and review the diff of the two
files line by line: it is the list of launches that moved.  tests/test_launch_sequences_host.py imports the builder and the
runner from this file.  (Recorded that way since: the pair step's "bwd-only" case, a backward call with grad_loss_bwd as its
one incoming gradient -- `R -1` before launch_unit_scatter_tiles accepted it, the scatter and the vertex launch after; no other
line moved.)

The driver links every other source of build.SOURCES too (unrecorded_sources()), for its cases that are run and not recorded
(``--unrecorded``; with ``--stream HEX`` every case hands that stream over and the recorder reports calls on any other:
tests/test_stream_record_host.py).  Neither option changes a line of the recorded table.

The sizes of a kernel's explicit arguments come from the code-object metadata (``.args``) of the device assembly
(``--cuda-device-only -S``); objects and argument tables are cached under tests/host/build/, one per source, keyed on the
source's content hash the way build.py keys the library's objects.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, "launch_sequences.json")
HOST = os.path.join(ROOT, "tests", "host")
CACHE = os.path.join(HOST, "build")  # git-ignored
SOURCES = ["raster_fwd.hip", "raster_bwd.hip", "raster_bwd_vc.hip", "warp.hip", "warp_tiles.hip", "pair_step.hip", "vertex_stage.hip"]
RUNS = {"cus256": ["--cus", "256"], "cus64": ["--cus", "64"]}
SOURCE_TABLES = {}  # source -> its kernel argument table, filled by build_driver


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    raise RuntimeError("no host C++ compiler found (set CXX)")


def parse_kernel_args(asm_text):
    """{mangled kernel name: [bytes of each explicit argument]} from the amdhsa.kernels metadata of a device assembly file."""
    out = {}
    at = asm_text.find("amdhsa.kernels:")
    if at < 0:
        return out
    sizes, size = [], None
    for line in asm_text[at:].splitlines()[1:]:
        m = re.match(r"\s+(?:- )?\.(\w+):\s*(.*)$", line)
        if not m:
            if line.startswith("amdhsa.") or line.startswith("..."):
                break
            continue
        key, value = m.group(1), m.group(2).strip()
        if key == "size":
            size = int(value)
        elif key == "value_kind":
            if not value.startswith("hidden_"):
                sizes.append(size)
        elif key == "name" and line.startswith("    .name"):  # (the kernel's own name, not an argument's)
            out[value.strip("'\"")] = sizes
            sizes = []
    return out


def unrecorded_sources():
    """Every other source of the library (build.SOURCES is the one list of them), linked as well, host-only like the recorded
    ones, for the cases that are run but not recorded (launch_record --unrecorded: every entry point on the caller's stream,
    tests/test_stream_record_host.py); their launch geometry is in no golden file.  Computed, so that a source added to the
    build is never outside the recorder's checks."""
    from handobjectconsist_amd import build

    assert set(SOURCES) <= set(build.SOURCES), "a recorded source the library is not built from"
    return [src for src in build.SOURCES if src not in SOURCES]


def build_driver(verbose=False):
    """-> (driver executable, kernel argument table); compiles what the cache under tests/host/build/ does not hold."""
    from handobjectconsist_amd import build

    os.makedirs(CACHE, exist_ok=True)
    hh = hashlib.sha256()
    for hdr in sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hpp", ".h"))) + [os.path.join("..", "..", "include", "meshraster_hip.h")]:
        with open(os.path.join(build.CSRC, hdr), "rb") as fh:
            hh.update(fh.read())
    procs, objs, tables = [], [], []
    tmp = ".%d.tmp" % os.getpid()  # (written under a name of this process, then renamed: concurrent builders do not collide)
    for src in SOURCES + unrecorded_sources():
        with open(os.path.join(build.CSRC, src), "rb") as fh:
            key = hashlib.sha256(" ".join(build.COMPILE_FLAGS).encode() + hh.digest() + fh.read()).hexdigest()[:16]
        stem = os.path.join(CACHE, "%s.%s" % (os.path.splitext(src)[0], key))
        obj, table, asm = stem + ".host.o", stem + ".args.txt", stem + ".s"
        objs.append(obj)
        tables.append(table)
        SOURCE_TABLES[src] = table
        for target, extra in ((obj, ["--cuda-host-only", "-c"]), (table, ["--cuda-device-only", "-S"])):
            if os.path.exists(target):
                continue
            out = obj + tmp + ".o" if target == obj else asm + tmp + ".s"
            cmd = [build._hipcc()] + build.COMPILE_FLAGS + extra + ["-o", out, os.path.join(build.CSRC, src)]
            if verbose:
                print(" ".join(cmd))
            procs.append((target, out, cmd, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
    for target, out, cmd, proc in procs:
        _, err = proc.communicate()
        if proc.returncode != 0:
            raise RuntimeError("%s\n%s" % (" ".join(cmd), err))
        if target.endswith(".o"):
            os.replace(out, target)
        else:
            with open(out) as fh:
                kernels = parse_kernel_args(fh.read())
            os.remove(out)
            with open(target + tmp, "w") as fh:
                for name in sorted(kernels):
                    fh.write("%s %d %s\n" % (name, len(kernels[name]), " ".join(map(str, kernels[name]))))
            os.replace(target + tmp, target)
    args_table = os.path.join(CACHE, "kernel_args.txt")
    with open(args_table + tmp, "w") as out:
        for table in tables:
            with open(table) as fh:
                out.write(fh.read())
    os.replace(args_table + tmp, args_table)
    # the driver and the recorder: the host compiler alone; the objects' fat binaries (one undefined symbol each) resolve to 0
    cxx = _host_compiler()
    h = hashlib.sha256((cxx + " ".join(objs)).encode())
    for f in ("hip_recorder.cpp", "launch_record_main.cpp"):
        with open(os.path.join(HOST, f), "rb") as fh:
            h.update(fh.read())
    exe = os.path.join(CACHE, "launch_record.%s" % h.hexdigest()[:16])
    if not os.path.exists(exe):
        nm = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True, check=True).stdout
        fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", nm)))
        cmd = ([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe + tmp,
                os.path.join(HOST, "launch_record_main.cpp"), os.path.join(HOST, "hip_recorder.cpp")] + objs
               + ["-Wl,--defsym=%s=0" % s for s in fatbins])
        if verbose:
            print(" ".join(cmd))
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            raise RuntimeError("%s\n%s" % (" ".join(cmd), done.stderr))
        os.replace(exe + tmp, exe)
    return exe, args_table  # (nothing is cleaned up here: another process may be linking against what this one does not need)


def run_driver(exe, args_table, extra=()):
    """The driver's output as {case name: [lines]} (insertion-ordered)."""
    done = subprocess.run([exe, args_table] + list(extra), capture_output=True, text=True)
    if done.returncode != 0:
        raise RuntimeError("launch_record %s: exit %d\n%s" % (" ".join(extra), done.returncode, done.stderr[-2000:]))
    return parse(done.stdout)


def parse(text):
    cases, lines = {}, None
    for line in text.splitlines():
        if line.startswith("# "):
            name = line[2:]
            assert name not in cases, "case named twice: " + name
            lines = cases[name] = []
        else:
            lines.append(line)
    return cases


def record(exe, args_table):
    return {run: run_driver(exe, args_table, extra) for run, extra in RUNS.items()}


def encode(runs, kernels):
    """The file's compact form of a record: {run: {entry point: {case: "line|line|..."}}}.  A launch names its kernel by its
    index in `kernels` (extended by the kernels not yet in it) and drops the grid's trailing ones."""
    out = {}
    for run, cases in runs.items():
        for name, lines in cases.items():
            entry, _, rest = name.partition(" ")
            packed = []
            for line in lines:
                f = line.split(" ")
                if f[0] in "LS" and len(f) > 2:
                    if f[1] not in kernels:
                        kernels.append(f[1])
                    f[1] = str(kernels.index(f[1]))
                    if f[0] == "L":
                        f[2] = re.sub(r"(,1)+$", "", f[2])
                    line = f[0] + " ".join(f[1:])
                packed.append(line)
            out.setdefault(run, {}).setdefault(entry, {})[rest] = "|".join(packed)
    return out


def decode(packed, kernels):
    """A case's lines as the driver printed them, for a message."""
    lines = []
    for line in packed.split("|"):
        m = re.match(r"([LS])(\d+) (.*)$", line)
        lines.append("%s %s %s" % (m.group(1), kernels[int(m.group(2))], m.group(3)) if m else line)
    return lines


def main():
    from handobjectconsist_amd import build

    exe, args_table = build_driver(verbose=True)
    runs = record(exe, args_table)
    if runs != record(exe, args_table):
        raise SystemExit("the recorder's output differs between two runs of one binary")
    kernels = []
    packed = encode(runs, kernels)
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as fh:
        fh.write('{\n "source_hash": %s,\n "kernels": %s,\n "runs": {\n' % (json.dumps(sys.argv[2] if len(sys.argv) > 2 else build.source_hash()),
                                                                           json.dumps(kernels)))
        for run in packed:
            fh.write('  %s: {\n' % json.dumps(run))
            for entry in packed[run]:
                rows = ",\n".join("%s:%s" % (json.dumps(case), json.dumps(seq)) for case, seq in packed[run][entry].items())
                fh.write('%s: {\n%s\n}%s\n' % (json.dumps(entry), rows, "," if entry != list(packed[run])[-1] else ""))
            fh.write('  }%s\n' % ("," if run != list(packed)[-1] else ""))
        fh.write(" }\n}\n")
    print(path, sum(len(v) for v in runs.values()), "cases,", sum(len(l) for v in runs.values() for l in v.values()), "lines,",
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
