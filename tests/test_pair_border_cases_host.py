"""The border cases of tests/pair_border_cases.py on the CPU, from the oracle alone: for every case and both of its seeds the
border classes are counted on the oracle's flows, masks and gradients and have to reach the case's conditions -- so that
tests/test_gpu_pair_borders.py cannot silently stop exercising a border --, W5's exact zeros are the oracle's, and every case
is one the fused path takes (V <= 2560, ``mr_pair_step_sizes`` answers MR_OK, csrc/launch_plan.hpp plans it with status 0),
so ``flow_pair_loss`` will not hand it to the composed path.  Which plan branch a case takes is printed, not asserted.

Classes (``pair_border_cases.classes``), summed over samples and both directions:
  out-L / -R / -T / -B   a non-zero flow whose bilinear sample has a tap beyond that side of the image
  edge-L / -R / -T / -B  a valid loss sample (``full_mask``) in the outermost column or row of that side
  off-grad               a vertex with |NDC x or y| > 1 and a non-zero oracle gradient
  occl-out               a flow that is non-zero before the occlusion step and zero after it, and whose nearest-neighbour sample
                         position lies outside the raster
"""
import ctypes
import subprocess

import numpy as np
import pytest

from handobjectconsist_amd.utils import synth
from oracle import raster_ref as R
from oracle import warp_ref as W
from tests import pair_border_cases as PB
from tests import pair_oracle_harness as H
from tests.test_launch_plan_host import _host_compiler
from tests.test_pair_mesh_cases_host import SOURCE

SEEDS = [(n, c["seed"] + d) for n, c in PB.CASES.items() for d in (0, PB.SECOND_SEED)]


def _counts(name, seed):
    case = PB.CASES[name]
    fwd, orc = H.oracle_forward(name, seed), H.oracle(name, seed)
    s = fwd["scene"]
    noocc = W.get_opticalflow(R, [s["verts1"], s["verts2"]], s["faces"], [s["K1"], s["K2"]], fwd["kw"], orig_img_size=None,
                              mask_occlusions=False, ignore_face_idxs=synth.HAND_IGNORE_FACES)
    g = orc["grads"]
    return PB.classes(case, fwd, noocc, orc["full_masks"], (np.concatenate(g[:2], 1), np.concatenate(g[2:], 1)), W, R)


@pytest.mark.parametrize("name,seed", SEEDS)
def test_each_case_reaches_its_border_classes(name, seed):
    case = PB.CASES[name]
    got = _counts(name, seed)
    print(f"{name} seed {seed}: " + ", ".join(f"{k} {v}" for k, v in got.items()) + f"; oracle {H.oracle(name, seed)['seconds']:.1f} s")
    short = {k: (v, case["conditions"][k]) for k, v in got.items() if v < case["conditions"][k]}
    assert not short, f"case {name}, seed {seed} no longer reaches (class: (count, needed)) {short}: retune its motion or seed"


def test_the_scene_keeps_the_parts_contract():
    for name, case in PB.CASES.items():
        s = PB.wall_scene(case)
        nh = synth.HAND_VERTS
        assert s["hand_faces"].max() < nh and s["obj_faces"].min() >= 0 and s["obj_faces"].max() < case["obj_verts"]
        assert s["obj_verts1"].shape == (case["B"], case["obj_verts"], 3) and s["obj_faces"].shape[1] == case["obj_face_rows"]
        assert (s["faces"][:, :synth.HAND_FACES] == s["hand_faces"]).all() and (s["faces"][:, synth.HAND_FACES:] == s["obj_faces"] + nh).all()
        # nothing at or behind the camera plane
        assert min(s["verts1"][..., 2].min(), s["verts2"][..., 2].min()) > 0.2, name
        im = PB.border_images(case, case["seed"])
        assert all(x.shape[2:] == (case["crop"][1], case["crop"][0]) for x in im)
        if case["jitter"] == "LT":
            assert not im[2][..., 0].any() and not im[2][..., 0, :].any() and im[2][..., 1:, 1:].all() and im[3][..., 1:, 1:].all()
        else:
            assert im[2].all() and im[3].all()


@pytest.mark.parametrize("name", list(PB.ZERO_SAMPLES))
@pytest.mark.parametrize("second", [False, True])
def test_a_frame_moved_off_screen_gives_exact_zeros(name, second):
    """a sample whose other frame is half a metre away: no warp sample lands in the image, the masked mean divides by 1, loss
    and gradient are exactly zero in the oracle (the device has to give exactly that); the ordinary sample is not zero"""
    case = PB.CASES[name]
    orc = H.oracle(name, case["seed"] + (PB.SECOND_SEED if second else 0))
    for b in range(case["B"]):
        zero = b in PB.ZERO_SAMPLES[name]
        assert (orc["lf"][b] == 0 and orc["lb"][b] == 0) == zero, (b, orc["lf"], orc["lb"])
        for g in orc["grads"]:
            assert np.isfinite(g).all() and (not g[b].any()) == zero, b


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_cases")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SOURCE], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    rows = [PB.plan_row(c) for c in PB.CASES.values()]
    run = subprocess.run([exe], input="".join(" ".join(str(v) for v in r) + "\n" for r in rows), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows), run.stdout
    return dict(zip(PB.CASES, lines))


@pytest.mark.parametrize("name", list(PB.CASES))
def test_the_fused_path_takes_every_case(decisions, name):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    case = PB.CASES[name]
    assert case["fused"]
    B2, V, Fh, Fo, _, is_ = PB.plan_row(case)
    assert V == synth.HAND_VERTS + case["n"] ** 2 and V <= 2560 and Fo == 2 * (case["n"] - 1) ** 2
    print(f"{name}: {decisions[name]}")
    fields = dict(item.split("=") for item in decisions[name].split())
    assert int(fields["status"]) == 0 and int(fields["scatter_status"]) == 0, decisions[name]
    st = pairstep.MrPairStep()
    sizes = dict(batch_size=case["B"], num_verts_a=synth.HAND_VERTS, num_verts_b=V - synth.HAND_VERTS, num_hand_faces=Fh, num_obj_faces=Fo,
                 fill_back=1, image_size=is_, height=case["crop"][1], width=case["crop"][0], jitter_channels=case["jitter_channels"])
    for k, v in sizes.items():
        setattr(st, k, v)
    sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert _lib.load().mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == 0
    assert sc.value > 0 and sv.value > 0
