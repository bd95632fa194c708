"""Every sizing entry point against tests/golden/workspace_sizes.json, value for value: the sizes, the offsets that
mr_render_tile_list and mr_pair_step_sizes hand out and the error codes of negative and zero arguments, as the library
answered them before the entry points' host side moved onto csrc/host_layout.hpp (one carved layout per workspace instead
of a size formula and a pointer walk written out separately).  tests/golden/make_golden_workspace_sizes.py holds the grid
and the runner; the file is never regenerated from later code.  No device is needed: the entry points are arithmetic."""
import importlib.util
import json
import os

import pytest

from handobjectconsist_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_golden_workspace_sizes", os.path.join(GOLDEN, "make_golden_workspace_sizes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "workspace_sizes.json")) as _fh:
    RECORD = json.load(_fh)

ENTRIES = sorted(list(gen.PLAIN) + ["mr_render_tile_list", "mr_pair_step_sizes", "mr_stem_conv_wrw_tiling"])


@pytest.fixture(scope="module")
def answers():
    return gen.run(_lib.load())


def test_record_covers_every_sizing_entry_point():
    """the record has exactly the generator's entry points and rows, and every int64-returning sizing symbol of the ABI is
    among them"""
    assert sorted(RECORD["entries"]) == ENTRIES
    assert len(RECORD["source_hash"]) == 64
    sizing = {n for n, (res, _) in _lib.SIGNATURES.items() if res is _lib._L and n != "mr_pair_step_struct_bytes"}
    assert sizing <= set(ENTRIES), sorted(sizing - set(ENTRIES))
    assert 2000 <= sum(len(v) for v in RECORD["entries"].values()) <= 5000
    # the example rows of the record's description
    assert [3, 5, 1536] in RECORD["entries"]["mr_render_backward_list_workspace_bytes"]
    assert [2, 10, 36, 0, 5120, 5632, 20] in RECORD["entries"]["mr_render_tile_list"]


@pytest.mark.parametrize("name", ENTRIES)
def test_sizes_match_the_record(answers, name):
    got, want = answers[name], RECORD["entries"][name]
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{name}: {len(wrong)} of {len(want)} rows differ (got, recorded), first: {wrong[:5]}"
