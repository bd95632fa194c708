"""The mesh cases of tests/pair_mesh_cases.py against csrc/launch_plan.hpp itself, on the CPU: tests/host/launch_plan_cases.cpp
(plain C++17, built with the host compiler as tests/test_launch_plan_host.py builds its program) prints what the binning pass
and the pair scatter decide for every case on a 256-CU device, and the tests assert that every mesh-dependent decision is
reached by a named case and that every case reaches the decision its row names.  A changed constant in launch_plan.hpp fails
here, with the case to move, instead of silently un-testing a branch of tests/test_gpu_pair_meshes.py.

Also here: the hand-written fused-path gate (``opticalflow._stacked_flow_node_ok``) against the library's
(``mr_pair_step_sizes``, pure arithmetic) on both sides of the vertex and raster limits, and the pair step's answers to an empty
batch and to a pair without an object -- all without a device."""
import ctypes
import os
import subprocess
import types

import pytest
import torch

from tests import pair_mesh_cases as P
from tests.test_launch_plan_host import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host", "launch_plan_cases.cpp")


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    """case name -> {field: value} of the program's line for it ("480": the existing 1 x 480 shape)"""
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_cases")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SOURCE], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    names = list(P.CASES) + ["480"]
    rows = [P.plan_row(P.CASES[n]) for n in P.CASES] + [P.plan_row(dict(P.EXISTING_480))]
    run = subprocess.run([exe], input="".join(" ".join(str(v) for v in r) + "\n" for r in rows), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows), run.stdout
    out = {}
    for name, line in zip(names, lines):
        d = dict(item.split("=") for item in line.split())
        out[name] = {k: (v if k == "sides" else int(v)) for k, v in d.items()}
        assert out[name]["status"] == 0, (name, line)
    return out


@pytest.mark.parametrize("name", list(P.CASES))
def test_each_case_reaches_the_decision_its_row_names(decisions, name):
    got = decisions[name]
    for field, want in P.CASES[name]["reach"].items():
        assert got[field] == want, (f"case {name} ({P.CASES[name]['note']}) no longer reaches {field} = {want!r} on a 256-CU device: "
                                    f"launch_plan.hpp now gives {got[field]!r}; move the case (tests/pair_mesh_cases.py)")
    # (the clamp as the parts themselves show it)
    if got["kh"] >= 0:
        assert got["hand_parts"] == got["kh"] and 1 <= got["kh"] <= got["parts"] - 1


def test_the_cases_cover_every_mesh_dependent_decision(decisions):
    fused = {n: d for n, d in decisions.items() if n != "480" and P.CASES[n]["fused"]}

    def reached(pred):
        return sorted(n for n, d in fused.items() if pred(d))

    cover = {
        **{f"parts {k}": reached(lambda d, k=k: d["parts"] == k) for k in (1, 2, 4, 8, 16)},
        "parts in one launch": reached(lambda d: d["parts"] > 1 and not d["two_launches"]),
        "count + fill launches": reached(lambda d: d["two_launches"] == 1),
        "boxes in LDS": reached(lambda d: d["lds_boxes"] == 1),
        "boxes beyond LDS": reached(lambda d: d["lds_boxes"] == 0 and d["faces"] == P.FACES_LAUNCH),
        "prologue in the kernel": reached(lambda d: d["prologue"] == P.PRO_IN_KERNEL),
        "prologue as a launch by plan": reached(lambda d: d["prologue"] == P.PRO_SEPARATE),
        "PROLOGUE within the default LDS": reached(lambda d: d["form"] == P.FORM_PROLOGUE and not d["lds_opt_in"]),
        "PROLOGUE with the LDS opt-in": reached(lambda d: d["form"] == P.FORM_PROLOGUE and d["lds_opt_in"] == 1 and d["lds"] > 48 * 1024),
        "Kh clamped down": reached(lambda d: d["kh_raw"] > d["kh"] >= 1),
        "Kh clamped up": reached(lambda d: 0 <= d["kh_raw"] < d["kh"]),
        "Kh unclamped": reached(lambda d: d["kh"] >= 1 and d["kh_raw"] == d["kh"]),
        "side -1 with a two-sided mesh": reached(lambda d: d["sides"] == "-1"),
        "8 scatter groups": reached(lambda d: d["groups"] == 8),
        "16 scatter groups": reached(lambda d: d["groups"] == 16),
        "odd V": sorted(n for n in fused if (P.plan_row(P.CASES[n])[1] & 1)),
        "even V": sorted(n for n in fused if not (P.plan_row(P.CASES[n])[1] & 1)),
    }
    for what, names in cover.items():
        print(f"{what}: {', '.join(names) or '-'}")
    missing = [what for what, names in cover.items() if not names]
    assert not missing, f"no case of tests/pair_mesh_cases.py reaches: {missing}"
    # two-sided: the one-part cases do have hand and object faces
    for n in cover["side -1 with a two-sided mesh"]:
        row = P.plan_row(P.CASES[n])
        assert row[2] > 0 and row[3] > 0
    # 32 groups: test_gpu_compact_batch.SHAPES' (1, 480, 270, 480, 3) on synth.random_scene's mesh
    from tests import test_gpu_compact_batch

    assert any(s[0] == P.EXISTING_480["B"] and s[1] == P.EXISTING_480["raster"] for s in test_gpu_compact_batch.SHAPES)
    assert decisions["480"]["groups"] == 32
    # the table limit: V = 2560 fills the colour-space table exactly, V = 2561 is past it (the flow-space table still fits)
    assert decisions["E"]["colour_table"] == 60 * 1024 and decisions["K"]["colour_status"] == -2 and decisions["K"]["scatter_status"] == 0


def _step(B, Va, Vb, Fh, Fo, is_):
    from handobjectconsist_amd.warping import pairstep

    st = pairstep.MrPairStep()
    sizes = dict(batch_size=B, num_verts_a=Va, num_verts_b=Vb, num_hand_faces=Fh, num_obj_faces=Fo, fill_back=1, image_size=is_, height=is_,
                 width=is_, jitter_channels=3)
    for k, v in sizes.items():
        setattr(st, k, v)
    return st


@pytest.mark.parametrize("V", [2559, 2560, 2561])
@pytest.mark.parametrize("is_", [252, 254, 256, 1024, 1028])
def test_the_python_gate_is_the_librarys(monkeypatch, V, is_):
    """opticalflow._stacked_flow_node_ok (written by hand) says "fused" exactly where mr_pair_step_sizes answers MR_OK, and
    where it says no the library answers MR_ERR_NOTIMPL (never BADARG: the composed path is the answer, not an error)."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import opticalflow

    monkeypatch.setattr(opticalflow, "USE_FLOW_RENDER", True)
    monkeypatch.setattr(opticalflow, "USE_STACKED_FLOW_NODE", True)
    ren = types.SimpleNamespace(image_size=is_, anti_aliasing=False)
    Vb = V - 778
    gate = bool(opticalflow._stacked_flow_node_ok(ren, V))
    st = _step(2, 778, Vb, 1552, 2 * Vb - 4, is_)
    sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = _lib.load().mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th))
    assert gate == (V <= 2560 and is_ in (252, 256, 1024)), "the gate moved: move this test's grid with it"
    assert rc == (0 if gate else -2), (V, is_, gate, rc)
    if gate:
        assert sc.value > 0 and sv.value > 0


def test_an_empty_batch_and_an_objectless_pair_take_the_composed_path():
    """pairstep.pair_step answers None -- "the fused path does not apply" -- for B == 0 (the struct call would return without
    writing, and losses[0] of an uninitialised buffer would be handed out as the batch mean) and for a pair without object
    vertices (mr_pair_step_sizes: MR_ERR_BADARG), before it touches a device; the library's answers are what they were."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    lib = _lib.load()
    assert lib.mr_pair_step_sizes(ctypes.byref(_step(2, 778, 0, 1552, 0, 64)), None, None, None) == -1
    assert lib.mr_pair_step_sizes(ctypes.byref(_step(0, 778, 4, 1552, 4, 64)), None, None, None) == 0

    def call(B, Vo):
        h, o = torch.zeros(B, 778, 3, requires_grad=True), torch.zeros(B, Vo, 3, requires_grad=True)
        im, jm = torch.zeros(B, 3, 64, 64), torch.ones(B, 3, 64, 64)
        K = torch.eye(3)[None].repeat(B, 1, 1)
        return pairstep.pair_step((h, o), (h, o), torch.zeros(1552, 3, dtype=torch.int64), torch.zeros(B, max(2 * Vo - 4, 0), 3, dtype=torch.int64),
                                  K, K, None, 64, 64, 64, im, im, jm, jm, None)

    before = dict(pairstep._PLANS)
    assert call(0, 4) is None and call(2, 0) is None and call(0, 0) is None
    assert pairstep._PLANS == before, "no plan is made for a pair the step does not take"
