"""The numpy warp oracle against the golden vectors captured from the REAL reference
(tests/golden/make_golden_warp.py imports /root/reference/meshreg/warping/imgflowarp.py etc.)."""
import os

import numpy as np

from oracle import warp_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_warp_bilinear_nearest_and_grads():
    g = np.load(os.path.join(GOLDEN, "warp_basic.npz"))
    for mode in ("bilinear", "nearest"):
        out, mask = W.warp(g["x"], g["flow"], mode=mode)
        assert (mask != g[f"mask_{mode}"]).sum() == 0
        assert np.abs(out - g[f"out_{mode}"]).max() < 2e-6
    gflow, gx = W.warp_backward(g["x"], g["flow"], g["grad_out"])
    assert np.abs(gflow - g["grad_flow"]).max() < 1e-5 * max(1, np.abs(g["grad_flow"]).max())
    assert np.abs(gx - g["grad_x"]).max() < 1e-5
    # flows include exactly-zero, integer, sub-pixel and far out-of-bounds vectors
    assert (g["flow"] == 0).any() and (np.abs(g["flow"]) > 500).any() and g["mask_bilinear"].min() == 0


def test_meshgrid():
    g = np.load(os.path.join(GOLDEN, "warp_basic.npz"))
    for s in (0, 1):
        assert np.array_equal(W.get_spatial_meshgrid(g["x"].shape, bool(s)), g[f"meshgrid_{s}"])


def test_occlusion_mask():
    g = np.load(os.path.join(GOLDEN, "warp_occlusion.npz"))
    o1, o2 = W.get_occlusion_mask(g["mask_flow1"], g["mask_flow2"], g["flow12"], g["flow21"])
    assert np.abs(o1 - g["occl1"]).max() < 1e-7 and np.abs(o2 - g["occl2"]).max() < 1e-7
    assert g["occl1"].sum() > 10 and (g["occl1"] == 0).any()


def test_pair_consist_loss_masks_grads():
    _pair_consist_against_the_reference("l1", "warp_pair_consist.npz")


def test_pair_consist_l2_loss_masks_grads():
    """the oracle's criterion="l2" against the reference's pair_consist with PyramidCriterion("l2") on the same inputs"""
    _pair_consist_against_the_reference("l2", "warp_pair_consist_l2.npz")


def _pair_consist_against_the_reference(criterion, fixture):
    g = np.load(os.path.join(GOLDEN, fixture))
    flows = [g["flow12"], g["flow21"]]
    args = (g["image_ref"], g["image"], g["jitter_ref"], g["jitter"])
    for ub in (0, 1):
        loss, masks, warps, diffs, _ = W.pair_consist(flows, *args, bool(ub), criterion=criterion)
        assert np.abs(loss - g[f"loss_ub{ub}"]).max() < 1e-6
        grads = W.pair_consist_grad(flows, *args, g["grad_loss"], bool(ub), criterion=criterion)
        for k, name in ((0, "grad_flow12"), (1, "grad_flow21")):
            ref = g[f"{name}_ub{ub}"]
            assert np.abs(grads[k] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-12) + 1e-9
    for i in (1, 2):
        assert (masks[i - 1]["warp_mask"] != g[f"warp_mask{i}"]).sum() == 0
        assert (masks[i - 1]["full_mask"] != g[f"full_mask{i}"]).sum() == 0
        assert (masks[i - 1]["flow_mask"] != g[f"flow_mask{i}"]).sum() == 0
        assert np.abs(warps[i - 1] - g[f"warp{i}"]).max() < 2e-6
        assert np.abs(diffs[i - 1] - g[f"diff{i}"]).max() < 2e-6
    assert g["loss_ub1"][2] == 0  # a sample with no valid pixel: masked mean divides by 1


def test_masked_mean():
    g = np.load(os.path.join(GOLDEN, "warp_misc.npz"))
    assert np.abs(W.batch_masked_mean_loss(g["dists"], g["mask"]) - g["masked_mean"]).max() < 1e-6
    assert g["masked_mean"][1] == 0


def _chain(name):
    import json

    z = np.load(os.path.join(GOLDEN, name))
    return z, json.loads(str(z["meta"]))


def _renderer_kw(is_):
    return dict(R=np.eye(3, dtype=np.float32)[None], t=np.zeros((1, 3), np.float32), dist_coeffs=np.zeros((1, 5), np.float32),
                orig_size=is_, image_size=is_, anti_aliasing=False, near=0.1, far=100, eps=1e-3, num_threads=4)


def _relerr(a, b):  # (test_oracle_chain.relerr: the largest error over the largest reference value)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def test_opticalflow_vertex_grad_matches_the_reference_run():
    """W.get_opticalflow_vertex_grad (float64; the oracle's own adjoint chain) against d loss / d vertices of both frames that
    the reference's get_opticalflow + autograd gave on the CPU (tests/golden/chain_opticalflow.npz: every variant of the
    training graph -- renders detached, textures attached, occlusion masks --; chain_opticalflow_cfg.npz: rasters of 480 and
    640 with the upstream gradients of make_golden_chain.flow_grad_inputs), at test_oracle_chain.py's tolerance for gradient
    arrays (1e-6 of the largest value; the fixtures are fp32 sums).  Both the float64 chain and its fp32 evaluation."""
    from oracle import raster_ref as R

    z, meta = _chain("chain_opticalflow.npz")
    ran = 0
    for m in meta:
        if not (m["detach_renders"] and m["mask_occlusions"]) or m["detach_textures"]:
            continue
        s, k, is_ = m["scene"], m["key"], m["image_size"]
        ignore = m["ignore_face_idxs"] if m["ignore"] else None
        args = (R, [z[f"{s}_verts1"], z[f"{s}_verts2"]], z[f"{s}_faces"], [z[f"{s}_K1"], z[f"{s}_K2"]], _renderer_kw(is_))
        flows = W.get_opticalflow(*args, orig_img_size=m["orig_img_size"], ignore_face_idxs=ignore)
        for i, name in enumerate(("flow12", "flow21")):  # (the same pixels carry a flow: the gradients are comparable)
            assert np.array_equal(flows[i] != 0, z[f"{k}_{name}"] != 0), (k, name)
        for fp32 in (False, True):
            grads = W.get_opticalflow_vertex_grad(*args, [z[f"{s}_g12"], z[f"{s}_g21"]], m["orig_img_size"], ignore, fp32=fp32)
            for g, name in zip(grads, ("grad_verts1", "grad_verts2")):
                want = z[f"{k}_{name}"]
                assert g.dtype == (np.float32 if fp32 else np.float64) and np.abs(want).max() > 0
                assert _relerr(g, want) < 1e-6, (k, name, fp32, _relerr(g, want))
        ran += 1
    assert ran >= 4
    z, meta = _chain("chain_opticalflow_cfg.npz")
    for m in meta:
        s, is_, (Wd, H), B = m["scene"], m["image_size"], m["orig_img_size"], m["batch"]
        r = np.random.default_rng(m["grad_seed"])  # = tests/golden/make_golden_chain.py::flow_grad_inputs
        g12, g21 = r.standard_normal((B, H, Wd, 2)).astype(np.float32), r.standard_normal((B, H, Wd, 2)).astype(np.float32)
        grads = W.get_opticalflow_vertex_grad(R, [z[f"{s}_verts1"], z[f"{s}_verts2"]], z[f"{s}_faces"], [z[f"{s}_K1"], z[f"{s}_K2"]],
                                              _renderer_kw(is_), [g12, g21], (Wd, H), m["ignore_face_idxs"])
        for g, name in zip(grads, ("grad_verts1", "grad_verts2")):
            assert _relerr(g, z[f"{s}_{name}"]) < 1e-6, (s, name, _relerr(g, z[f"{s}_{name}"]))
