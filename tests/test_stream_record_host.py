"""Every runtime call of every entry point goes to the stream the caller handed over.  No device: every source of build.SOURCES,
host-only, on tests/host/hip_recorder.cpp, which keeps the stream of each hipLaunchKernel, hipMemsetAsync, hipMallocAsync and
hipFreeAsync and prints an `X` line for a call on another stream than the one the driver announced.

launch_record --stream 0x5eed00 hands that made-up stream to every case of the recorded table; --unrecorded adds the cases
whose launch geometry no golden file holds: the entry points of every source the table does not record (gen.unrecorded_sources():
whatever else the library is built from), the entry points of the seven recorded sources the table never calls, and
the shapes that pick the remaining strip instantiations of kernel D.  A launcher that sent one launch or memset to stream 0
-- a race on a side stream, a node missing from a captured graph -- shows as an X line here.

(The raster-orientation instantiations of strip_gather_kernel, nine kernels no entry point could select, were found by the
never-launched list below and are no longer instantiated: raster_bwd.hip, launch_pixel_map.)"""
import importlib.util
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_launch_sequences", os.path.join(HERE, "golden", "make_golden_launch_sequences.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

SENTINEL = ["--stream", "0x5eed00"]
SELFTEST = "selftest: expectation differs from the stream handed over"
NEVER = "never launched"

# Kernels of the seven recorded sources that no case launches, each with the reason no case can: an instantiation that only a
# profiling or debug flag selects, or one that only a device property other than the CU count selects.  "No case yet" is no
# reason.  (Empty: every registered kernel of every source is launched.)
NEVER_LAUNCHED = {}
# Sources without a kernel of their own: host code only.  Every other unrecorded source must bring at least one.
HOST_ONLY = {"library.hip"}  # mr_abi_version and mr_device_ok: no launch, no stream


@pytest.fixture(scope="module")
def driver():
    return gen.build_driver()


@pytest.fixture(scope="module")
def sentinel_runs(driver):
    return {run: gen.run_driver(*driver, extra + SENTINEL + ["--unrecorded"]) for run, extra in gen.RUNS.items()}


def _kinds(lines, kinds="LMAF"):
    return [l for l in lines if l[:2] in tuple(k + " " for k in kinds)]


@pytest.mark.parametrize("run", sorted(gen.RUNS))
def test_the_stream_changes_no_decision_and_every_call_is_on_it(driver, run):
    plain = gen.run_driver(*driver, gen.RUNS[run])
    on_stream = gen.run_driver(*driver, gen.RUNS[run] + SENTINEL)
    off = [(name, l) for name, lines in on_stream.items() for l in lines if l.startswith("X ")]
    assert not off, "calls off the caller's stream: %s" % off[:10]
    assert len(_kinds([l for lines in plain.values() for l in lines])) > 250
    assert on_stream == plain


@pytest.mark.parametrize("run", sorted(gen.RUNS))
def test_unrecorded_cases_stay_on_the_stream(sentinel_runs, run):
    cases = sentinel_runs[run]
    new = {name: lines for name, lines in cases.items() if name.startswith("unrecorded ")}
    assert len(new) > 170
    refused = [name for name, lines in new.items() if lines[-1] != "R 0"]
    assert not refused, "cases the entry point refused launch nothing: %s" % refused
    idle = [name for name, lines in new.items() if not _kinds(lines) and " B0" not in name]
    assert not idle, "cases without a runtime call: %s" % idle
    off = [(name, l) for name, lines in cases.items() if name != SELFTEST for l in lines if l.startswith("X ")]
    assert not off, "calls off the caller's stream: %s" % off[:10]


def test_the_check_can_fail(sentinel_runs):
    """One case hands over 0x5eed00 while the recorder expects 0x5eed10: every call of it is reported, and the case makes
    all four kinds of call."""
    lines = sentinel_runs["cus256"][SELFTEST]
    calls, off = _kinds(lines), [l for l in lines if l.startswith("X ")]
    assert len(off) == len(calls) >= 4
    assert {l.split()[1] for l in off} == set("LMAF")
    assert {l[0] for l in calls} == set("LMAF")
    assert all(l.split()[-1] == "0x5eed00" for l in off)
    # each X line stands in front of the line of its call
    for x, call in zip(off, calls):
        assert lines.index(x) + 1 == lines.index(call) and x.split()[1] == call[0]


def test_no_x_or_u_lines_without_being_asked(driver):
    plain = gen.run_driver(*driver, gen.RUNS["cus256"])
    assert not [l for lines in plain.values() for l in lines if l[:2] in ("X ", "U ")]
    assert NEVER not in plain and SELFTEST not in plain


def _kernel_names(driver):
    """{source: set of kernel names as the L lines show them}, from each source's own argument table."""
    exe, args_table = driver
    out = {}
    for src, table in gen.SOURCE_TABLES.items():
        done = subprocess.run([exe, table, "--kernel-names"], capture_output=True, text=True, check=True)
        out[src] = {l.split(" ", 2)[2] for l in done.stdout.splitlines() if l.startswith("K ")}
    return out


@pytest.mark.parametrize("run", sorted(gen.RUNS))
def test_every_kernel_is_launched(driver, sentinel_runs, run):
    cases = sentinel_runs[run]
    launched = {l.split()[1] for lines in cases.values() for l in lines if l.startswith("L ")}
    names = _kernel_names(driver)
    from handobjectconsist_amd import build

    unrecorded = gen.unrecorded_sources()
    assert sorted(gen.SOURCES + unrecorded) == sorted(build.SOURCES) == sorted(names)
    for src in unrecorded:
        assert bool(names[src]) != (src in HOST_ONLY), src
        assert not names[src] - launched, "%s: never launched: %s" % (src, sorted(names[src] - launched))
    never = {l[2:] for l in cases[NEVER]}
    assert all(l.startswith("U ") for l in cases[NEVER])
    assert never == set(NEVER_LAUNCHED), "never launched, and not in the reasoned list: %s; listed, but launched: %s" % (
        sorted(never - set(NEVER_LAUNCHED)), sorted(set(NEVER_LAUNCHED) - never))
    recorded = set().union(*(names[src] for src in gen.SOURCES))
    assert not (recorded - launched) - set(NEVER_LAUNCHED)
    assert len(recorded) >= 90 and len(launched) >= len(recorded)


def test_unrecorded_cases_do_not_depend_on_the_run(driver):
    """The two-stack-fill property of test_record_does_not_depend_on_the_run for the new cases: argument blocks with
    uninitialised padding would hash to what the stack held.  (It found such blocks in mr_flow_vertices_forward, the two
    parts calls, mr_stack_pair_faces, the block tail, the colour augmentation and the general MANO call; they are
    value-initialised now.  The cases of mano_adapt, eval_metrics and frame_resize, under the recorder since the
    source list is computed, brought none: their blocks were value-initialised already.)

    One launch is left out, by its kernel's name: pair_prologue_kernel as mr_flow_pair_prologue_parts launches it.  The four
    bytes behind the last field of its StackFacesParams are not initialised, and tests/golden/launch_sequences.json holds the
    hash of that launch as the pair step makes it, with the byte the recorded tree's stack held there (0x20).  Initialising
    them changes that file, which is re-recorded only by a decision of its own; called directly, the launch's hash follows
    the stack fill.  Everything else of those cases is compared."""
    a = gen.run_driver(*driver, SENTINEL + ["--unrecorded", "--stack-fill", "0"])
    b = gen.run_driver(*driver, SENTINEL + ["--unrecorded", "--stack-fill", "165"])
    left_out = 0
    for cases in (a, b):
        for name, lines in cases.items():
            if name.startswith("unrecorded flow_pair_prologue_parts "):
                for i, l in enumerate(lines):
                    if l.startswith("L pair_prologue_kernel "):
                        lines[i] = l.rsplit(" ", 1)[0]
                        left_out += 1
    assert left_out == 2 * 4
    assert a == b
