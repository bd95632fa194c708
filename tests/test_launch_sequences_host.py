"""The raster and warp launchers against tests/golden/launch_sequences.json, line for line: every kernel, grid, block, dynamic
LDS size, argument hash, memset, allocation and attribute call of every case of tests/host/launch_record_main.cpp, as the
launchers made them before their decisions moved into csrc/launch_plan.hpp.  No device: the launchers' host-only objects run
on tests/host/hip_recorder.cpp (tests/golden/make_golden_launch_sequences.py builds the program from the tree at hand and
caches the objects under tests/host/build/)."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_golden_launch_sequences", os.path.join(GOLDEN, "make_golden_launch_sequences.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "launch_sequences.json")) as _fh:
    RECORD = json.load(_fh)


@pytest.fixture(scope="module")
def driver():
    return gen.build_driver()


def test_golden_file_is_a_record_of_one_source_tree():
    assert len(RECORD["source_hash"]) == 64
    assert set(RECORD["runs"]) == set(gen.RUNS)
    assert os.path.getsize(os.path.join(GOLDEN, "launch_sequences.json")) <= os.path.getsize(os.path.join(GOLDEN, "workspace_sizes.json"))


@pytest.mark.parametrize("run", sorted(gen.RUNS))
def test_every_launch_matches_the_record(driver, run):
    kernels = list(RECORD["kernels"])
    now = gen.encode({run: gen.run_driver(*driver, gen.RUNS[run])}, kernels)[run]
    then = RECORD["runs"][run]
    assert {e: list(c) for e, c in now.items()} == {e: list(c) for e, c in then.items()}, "the table of cases changed"
    wrong = []
    for entry, cases in then.items():
        for case, seq in cases.items():
            if now[entry][case] != seq:
                wrong.append("%s %s\n  recorded: %s\n  now:      %s" % (entry, case, "\n            ".join(gen.decode(seq, kernels)),
                                                                     "\n            ".join(gen.decode(now[entry][case], kernels))))
    assert not wrong, "%d of %d cases differ\n%s" % (len(wrong), sum(map(len, then.values())), "\n".join(wrong[:20]))


def test_record_does_not_depend_on_the_run(driver):
    """Two runs of one binary over stacks filled with different bytes: a parameter block with uninitialised padding would
    hash to what the stack held."""
    a = gen.run_driver(*driver, ["--stack-fill", "0"])
    b = gen.run_driver(*driver, ["--stack-fill", "165"])
    assert a == b


def test_lds_opt_in_is_raised_once_on_each_device(driver):
    """hipFuncSetAttribute acts on the current device: the same large launch twice on each of two devices raises the limit of
    the eight binning kernels once per device."""
    cases = gen.run_driver(*driver, ["--two-devices"])
    assert len(cases) == 4
    raised = {name: [l for l in lines if l.startswith("S ")] for name, lines in cases.items()}
    for dev in (0, 1):
        first, second = raised["two devices: round 0 device %d" % dev], raised["two devices: round 1 device %d" % dev]
        assert len(first) == 8 and all(l.endswith(" 8 155648 d%d" % dev) for l in first), first
        assert len({l.split()[1] for l in first}) == 8
        assert second == []
    launches = [[l for l in lines if l.startswith("L ")] for lines in cases.values()]
    assert all(l == launches[0] for l in launches)
