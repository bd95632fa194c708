"""The l2 photometric criterion (PyramidCriterion("l2"): torch.nn.MSELoss(reduction="none") + the per-sample masked mean,
pyramidloss.py:56-62, lossutils.py:1-8) on the fused pair-loss kernels (ABI 9, MR_CRITERION_L2): the dense and tile-list
pair kernels, the fused pair node in its unit / recompute forms and the struct path, against fixtures produced by running
the reference's own code (tests/golden/make_golden_l2.py) and against the composed path; l1 through the old entry points
and through the *_crit ones with MR_CRITERION_L1 bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from handobjectconsist_amd.utils import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a, dev, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return x.requires_grad_(True) if grad else x


def n(x):
    return x.detach().cpu().numpy()


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e}, {(err > tol).sum()} / {err.size} out of tol"


def norm_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _record_calls(monkeypatch):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    calls = []
    real_call, real_step = _lib.call, pairstep.pair_step
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(pairstep, "pair_step", lambda *a, **k: (calls.append("pair_step"), real_step(*a, **k))[1])
    return calls


class _Composed:
    """A criterion the fused kernels do not recognise (imgflowarp._fused_criterion -> None): the composed `warp` path with
    the reference's control flow, computing the same squared residuals as PyramidCriterion("l2")."""

    level_nb = 1

    def __init__(self):
        from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion

        self._inner = PyramidCriterion("l2")
        self.criterion = lambda a, b: (a - b) ** 2

    def compute(self, inp, target, mask=None):
        return self._inner.compute(inp, target, mask)


def _renderer(is_, dev):
    from handobjectconsist_amd.neurender.renderer import Renderer

    return Renderer(image_size=is_, R=torch.eye(3, device=dev).unsqueeze(0), t=torch.zeros(1, 3, device=dev),
                    K=torch.ones(1, 3, 3, device=dev), orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1,
                    no_light=True)


# ---------------------------------------------------------------------------------------------------
# 1. dense pair kernel against the reference
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("use_backward", [False, True])
def test_dense_pair_kernel_l2_golden(cuda, monkeypatch, use_backward):
    """pair_consist(..., PyramidCriterion("l2"), outputs="full") on the fused dense kernels (mr_pair_consist_*_crit) against
    the reference's pair_consist: losses and flow gradients at the l1 golden test's tolerances, masks exactly, warps and
    squared differences."""
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    g = np.load(os.path.join(GOLDEN, "warp_pair_consist_l2.npz"))
    calls = _record_calls(monkeypatch)
    tag = f"ub{int(use_backward)}"
    f12, f21 = t(g["flow12"], cuda, True), t(g["flow21"], cuda, True)
    loss, masks, warps, diffs = imgflowarp.pair_consist(
        [f12, f21], t(g["image_ref"], cuda), t(g["image"], cuda), t(g["jitter_ref"], cuda), t(g["jitter"], cuda),
        PyramidCriterion("l2"), use_backward=use_backward, outputs="full")
    close(n(loss), g[f"loss_{tag}"], 1e-5, 1e-7, "loss")
    assert float(g[f"loss_{tag}"][2]) == 0.0 and float(loss[2]) == 0.0  # (the sample without a valid pixel)
    (loss * t(g["grad_loss"], cuda)).sum().backward()
    g12 = n(f12.grad) if f12.grad is not None else np.zeros_like(g["flow12"])
    close(g12, g[f"grad_flow12_{tag}"], 1e-4, 1e-7, "grad_flow12")
    close(n(f21.grad), g[f"grad_flow21_{tag}"], 1e-4, 1e-7, "grad_flow21")
    assert np.abs(g[f"grad_flow21_{tag}"]).max() > 0
    assert "mr_pair_consist_forward_crit" in calls and "mr_pair_consist_backward_crit" in calls, calls
    assert "mr_warp_forward" not in calls, "the composed path ran"
    for i in (0, 1):
        assert (n(masks[i]["full_mask"]) != g[f"full_mask{i + 1}"]).sum() == 0
        assert (n(masks[i]["warp_mask"]) != g[f"warp_mask{i + 1}"]).sum() == 0
        assert (n(masks[i]["flow_mask"]) != g[f"flow_mask{i + 1}"]).sum() == 0
        close(n(warps[i]), g[f"warp{i + 1}"], 1e-5, 2e-6, "warp")
        close(n(diffs[i]), g[f"diff{i + 1}"], 1e-5, 2e-6, "squared diff")


# ---------------------------------------------------------------------------------------------------
# 2. tile-list kernels on sparse flows against the dense ones
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("B,is_,H,Wd", [(3, 256, 256, 256), (2, 96, 64, 96)])
def test_tile_list_kernels_l2_equal_dense(cuda, monkeypatch, B, is_, H, Wd):
    """get_opticalflow(sparse_flows=True) -> pair_consist(l2, outputs="loss") (mr_pair_consist_*_tiles_crit over the render's
    tile list, NaN-poisoned buffers) against the dense flows of the same meshes -> pair_consist(l2, outputs="full"):
    losses to fp32 rounding of the per-tile sums, vertex gradients of both frames."""
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp, opticalflow

    s = synth.random_scene(B, seed=7, image_size=is_)
    ren = _renderer(is_, cuda)
    im_ref, im, jm_ref, jm = [t(a, cuda) for a in synth.random_images(B, H, Wd, 5)]
    crit = PyramidCriterion("l2")
    weights = torch.linspace(0.5, 1.5, B, device=cuda)
    monkeypatch.setattr(opticalflow, "DEBUG_POISON_RENDER_OUTPUTS", True)
    monkeypatch.setattr(imgflowarp, "DEBUG_POISON_SPARSE_GRADS", True)
    calls = _record_calls(monkeypatch)

    def run(sparse):
        v1, v2 = t(s["verts1"], cuda, True), t(s["verts2"], cuda, True)
        flows = opticalflow.get_opticalflow([v1, v2], t(s["faces"], cuda), [t(s["K1"], cuda), t(s["K2"], cuda)], ren,
                                            orig_img_size=(Wd, H), detach_textures=False, detach_renders=True,
                                            ignore_face_idxs=synth.HAND_IGNORE_FACES, sparse_flows=sparse)
        loss = imgflowarp.pair_consist(flows, im_ref, im, jm_ref, jm, crit, use_backward=True,
                                       outputs="loss" if sparse else "full")[0]
        (loss * weights).sum().backward()
        return loss.detach(), v1.grad, v2.grad

    loss_d, g1_d, g2_d = run(False)
    assert "mr_pair_consist_forward_crit" in calls and "mr_pair_consist_backward_crit" in calls
    del calls[:]
    loss_s, g1_s, g2_s = run(True)
    for name in ("mr_pair_consist_forward_tiles_crit", "mr_pair_consist_backward_tiles_crit"):
        assert name in calls, (name, calls)
    assert float(loss_d.abs().sum()) > 0 and float(g1_d.abs().sum()) > 0
    close(n(loss_s), n(loss_d), 2e-6, 1e-9, "pair loss")
    for a, b_, what in ((g1_s, g1_d, "d/d vertices of frame 1"), (g2_s, g2_d, "d/d vertices of frame 2")):
        assert torch.isfinite(a).all(), what
        close(n(a), n(b_), 1e-5, 1e-6 * float(b_.abs().max()), what)


# ---------------------------------------------------------------------------------------------------
# 3. the metric workload in the trainer's mode against the reference
# ---------------------------------------------------------------------------------------------------


def _metric_inputs(z, m, dev):
    s = synth.random_scene(m["batch"], seed=m["scene_seed"], image_size=m["image_size"])
    im_ref, im, jm_ref, jm = synth.random_images(m["batch"], m["image_size"], m["image_size"], m["scene_seed"])
    got = dict(verts1=s["verts1"], verts2=s["verts2"], K1=s["K1"], faces=s["faces"], image0=im, image1=im_ref, jitter0=jm,
               jitter1=jm_ref)
    for k, v in got.items():
        assert float(np.asarray(v, np.float64).sum()) == float(z["checksum_" + k]), f"input {k} differs from the fixture's"
    B = m["batch"]
    samples, results = [], []
    for k, (img, jit) in enumerate(((im, jm), (im_ref, jm_ref))):
        f = "12"[k]
        samples.append({"image": t(img, dev), "jittermask": t(jit, dev), "camintr": t(s["K" + f], dev),
                        "objfaces": t(s["obj_faces"][None].repeat(B, 0), dev), "objverts3d": t(s["obj_verts" + f], dev),
                        "handverts3d": t(s["hand_verts" + f], dev)})
    results.append({"recov_handverts3d": t(s["hand_verts1"], dev, True), "recov_objverts3d": t(s["obj_verts1"], dev, True)})
    results.append({"recov_handverts3d": t(z["pred1_hand"], dev, True), "recov_objverts3d": t(z["pred1_obj"], dev, True)})
    return s, samples, results


@pytest.mark.parametrize("mode", ["step", "unit", "recompute"])
def test_metric_workload_training_mode_l2_against_the_reference(cuda, monkeypatch, mode):
    """warpbranch.forward as the trainer calls it (pair_outputs="loss") with PyramidCriterion("l2"), on NaN-poisoned render
    outputs: the pair is the fused node -- the struct path (``step``), or the node pair with the pair loss's gradient formed
    by the forward launch (``unit``) or recomputed by the backward launch (``recompute``) -- and the loss, the per-sample
    pair losses, d loss / d predicted vertices of frame 0 and the flows (where the reference's are non-zero) are the
    reference's."""
    from handobjectconsist_amd.models import warpbranch
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import opticalflow

    z = np.load(os.path.join(GOLDEN, "chain_metric_l2.npz"))
    m = json.loads(str(z["meta"]))
    assert m["criterion"] == "l2"
    B, is_ = m["batch"], m["image_size"]
    unit = mode != "recompute"
    monkeypatch.setattr(opticalflow, "USE_UNIT_GRADIENT", unit)
    monkeypatch.setattr(opticalflow, "USE_PAIR_STEP", mode == "step")
    monkeypatch.setattr(opticalflow, "DEBUG_POISON_RENDER_OUTPUTS", True)
    calls = _record_calls(monkeypatch)
    s, samples, results = _metric_inputs(z, m, cuda)
    loss, pair = warpbranch.forward(samples, results, t(s["hand_faces"], cuda)[None], _renderer(is_, cuda), (is_, is_),
                                    PyramidCriterion("l2"), gt_refs=True, first_only=True,
                                    hand_ignore_faces=m["hand_ignore_faces"], use_backward=True, pair_outputs="loss")
    loss.backward()
    fwd, bwd = (("mr_flow_pair_forward_grad_tiles_crit", "mr_flow_pair_backward_unit_tiles") if unit
                else ("mr_flow_pair_forward_tiles_crit", "mr_flow_pair_backward_tiles_crit"))
    if mode == "step":
        assert "pair_step" in calls and fwd not in calls, ("the trainer's setting must take the struct path", calls)
    else:
        assert fwd in calls and bwd in calls and "pair_step" not in calls, ("the fused pair node must run", calls)
    assert "mr_warp_forward" not in calls, "the composed path ran"
    assert all(x is None for x in pair["masks"]) and all(x is None for x in pair["warps"])
    for d in (0, 1):
        got = n(pair["recons_flows"][0][d]).reshape(-1, 2)
        idx, want = z[f"wb_flow{d}_idx"], z[f"wb_flow{d}_sample"]
        on = want[:, 0] != 0
        assert on.any() and np.abs(got[idx][on] - want[on]).max() <= 1e-6 * max(np.abs(want).max(), 1.0), ("flow", d)
    assert norm_rel(n(pair["diff_losses"]), z["wb_diff_losses"]) < 1e-5, (n(pair["diff_losses"]), z["wb_diff_losses"])
    assert abs(float(loss) - float(z["wb_loss"])) < 1e-5 * abs(float(z["wb_loss"])), (float(loss), float(z["wb_loss"]))
    for name, key in (("recov_handverts3d", "wb_grad_hand0"), ("recov_objverts3d", "wb_grad_obj0")):
        assert np.abs(z[key]).max() > 0
        assert norm_rel(n(results[0][name].grad), z[key]) < 1e-4, (key, norm_rel(n(results[0][name].grad), z[key]))
        assert results[1][name].grad is None, "the annotated frame must not receive a gradient"


# ---------------------------------------------------------------------------------------------------
# 4. WarpRegNet end to end: the trainer's "loss" outputs against "full"
# ---------------------------------------------------------------------------------------------------


def test_warpregnet_l2_loss_outputs_equal_full(cuda):
    """WarpRegNet(criterion="l2") with pair_outputs="loss" (the fused pair node) and "full" (dense flows, dense pair
    kernels, per-pixel outputs) on one consist batch of the trainer fixture: same loss, same parameter gradient at the
    trainer tests' tolerances."""
    from test_gpu_trainer import _KEYS, _trainer_batches
    from trainer_fake import FakeMeshRegNet

    from handobjectconsist_amd.models.warpreg import WarpRegNet

    zt = np.load(os.path.join(GOLDEN, "chain_trainer.npz"))
    cfg = json.loads(str(zt["meta"]))
    batch = _trainer_batches(zt, cfg, cuda)[1]
    assert batch["supervision"] == "consist"
    out = {}
    for outputs in ("loss", "full"):
        model = FakeMeshRegNet(_KEYS).to(cuda)
        is_ = cfg["image_size"]
        pre = WarpRegNet((is_, is_), model, lambda_data=cfg["lambda_data"], lambda_consist=cfg["lambda_consist"],
                         criterion="l2", progressive_steps=cfg["progressive_steps"], use_backward=True, gt_refs=True,
                         mano_faces=torch.from_numpy(synth.hand_template()[1][:1538].copy()), pair_outputs=outputs).to(cuda)
        pre.step_count = 3
        model.zero_grad()
        loss, agg, _, pair = pre.forward(batch)
        loss.sum().backward()
        assert pair is not None
        out[outputs] = (n(loss).reshape(-1), float(agg["warp_consist"]), n(model.w.grad))
    (l_loss, c_loss, g_loss), (l_full, c_full, g_full) = out["loss"], out["full"]
    assert c_full > 0
    assert norm_rel(l_loss, l_full) < 1e-5, (l_loss, l_full)
    assert abs(c_loss - c_full) <= 1e-5 * abs(c_full), (c_loss, c_full)
    assert np.abs(g_full).max() > 0 and norm_rel(g_loss, g_full) < 1e-4, (g_loss, g_full)


# ---------------------------------------------------------------------------------------------------
# 5. l1 unchanged: the old entry points and the *_crit ones with MR_CRITERION_L1 bit for bit
# ---------------------------------------------------------------------------------------------------


def test_l1_old_and_crit_entry_points_bit_identical(cuda, monkeypatch):
    """Every l1 call of the pair path through the entry points of ABI 8 (what the package calls for l1) and through their
    *_crit forms with MR_CRITERION_L1.  The dense pair kernels on leaf flows: losses
    and flow gradients bit for bit.  get_opticalflow -> the dense / tile-list kernels and the fused node in its unit and
    recompute forms: losses bit for bit, vertex gradients to the order of the raster backward's final fp32 atomics."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp, opticalflow

    B, is_ = 2, 96
    s = synth.random_scene(B, seed=11, image_size=is_)
    ren = _renderer(is_, cuda)
    im_ref, im, jm_ref, jm = [t(a, cuda) for a in synth.random_images(B, is_, is_, 4)]
    crit = PyramidCriterion("l1")
    real_call = _lib.call
    seen = []

    def crit_names(name, *a):  # the ABI 8 entry point -> its *_crit form with MR_CRITERION_L1
        if name + "_crit" in _lib.SIGNATURES:
            seen.append(name)
            return real_call(name + "_crit", *a, _lib.CRITERION_L1)
        return real_call(name, *a)

    def run(how):
        v1, v2 = t(s["verts1"], cuda, True), t(s["verts2"], cuda, True)
        args = ([v1, v2], t(s["faces"], cuda), [t(s["K1"], cuda), t(s["K2"], cuda)], ren)
        if how in ("dense", "tiles"):
            flows = opticalflow.get_opticalflow(*args, orig_img_size=(is_, is_), detach_textures=False, detach_renders=True,
                                                ignore_face_idxs=synth.HAND_IGNORE_FACES, sparse_flows=how == "tiles")
            loss = imgflowarp.pair_consist(flows, im_ref, im, jm_ref, jm, crit, use_backward=True,
                                           outputs="loss" if how == "tiles" else "full")[0]
        else:
            monkeypatch.setattr(opticalflow, "USE_UNIT_GRADIENT", how == "unit")
            lf, lb, _ = opticalflow.flow_pair_loss(*args, (is_, is_), im_ref, im, jm_ref, jm,
                                                   ignore_face_idxs=synth.HAND_IGNORE_FACES)
            loss = lf + lb
        (loss * torch.linspace(0.5, 1.5, B, device=cuda)).sum().backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), v1.grad.clone(), v2.grad.clone()

    def run_leaf():
        with torch.no_grad():
            flows = opticalflow.get_opticalflow([t(s["verts1"], cuda), t(s["verts2"], cuda)], t(s["faces"], cuda),
                                                [t(s["K1"], cuda), t(s["K2"], cuda)], ren, orig_img_size=(is_, is_),
                                                ignore_face_idxs=synth.HAND_IGNORE_FACES)
        f12, f21 = flows[0].detach().clone().requires_grad_(True), flows[1].detach().clone().requires_grad_(True)
        loss = imgflowarp.pair_consist([f12, f21], im_ref, im, jm_ref, jm, crit, use_backward=True, outputs="full")[0]
        (loss * torch.linspace(0.5, 1.5, B, device=cuda)).sum().backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), f12.grad.clone(), f21.grad.clone()

    for how in ("leaf", "dense", "tiles", "unit", "recompute"):
        fn = run_leaf if how == "leaf" else (lambda: run(how))
        monkeypatch.setattr(_lib, "call", real_call)
        new = fn()
        monkeypatch.setattr(_lib, "call", crit_names)
        del seen[:]
        old = fn()
        assert seen, f"{how}: no entry point with a *_crit form was called"
        assert float(new[0].abs().sum()) > 0 and float(new[1].abs().sum()) > 0
        assert torch.equal(new[0], old[0]), (how, "loss")
        for a, b_, what in zip(new[1:], old[1:], ("gradient 1", "gradient 2")):
            if how == "leaf":
                assert torch.equal(a, b_), (how, what)
            else:
                close(n(a), n(b_), 1e-6, 1e-7 * float(b_.abs().max()), f"{how}: {what}")


def test_unknown_criterion_is_a_bad_argument(cuda):
    """A criterion code the kernels have no instantiation for is MR_ERR_BADARG before any launch."""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    B, H, W = 1, 8, 8
    f = torch.zeros((B, H, W, 2), device=cuda)
    im = torch.zeros((B, 3, H, W), device=cuda)
    wbytes = int(lib.mr_pair_consist_workspace_bytes(B, H, W))
    work = torch.empty((wbytes,), dtype=torch.uint8, device=cuda)
    sums, lf, lb = torch.empty((B, 4), device=cuda), torch.empty((B,), device=cuda), torch.empty((B,), device=cuda)
    p = _lib.ptr
    head = (p(f), p(f), p(im), p(im), p(im), p(im), 3, p(work), wbytes, p(sums), p(lf), p(lb)) + (None,) * 8
    tail = (B, H, W, 0.99999, None, None, 0, _lib.stream_ptr(cuda))
    assert lib.mr_pair_consist_forward_crit(*head, *tail, 2) == -1
    assert lib.mr_pair_consist_forward_crit(*head, *tail, -1) == -1
    assert lib.mr_pair_consist_forward_crit(*head, *tail, _lib.CRITERION_L2) == 0
    torch.cuda.synchronize()
    assert torch.equal(lf, torch.zeros_like(lf))  # (all-zero flows: no valid pixel)


# ---------------------------------------------------------------------------------------------------
# 6. a short randomised slice: fused l2 against the composed l2 path
# ---------------------------------------------------------------------------------------------------


def test_l2_fused_equals_composed_random_shapes(cuda):
    """Random B, H, W -- odd sizes and W == 2 included -- with random sub-pixel flows (zeros, integer offsets, far
    vectors): the fused l2 kernels (dense, with their per-pixel outputs) against the composed warp path computing the
    same squared residuals: losses, flow gradients, masks, warps, squared differences."""
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    rng = np.random.default_rng(1234)
    shapes = [(1, 5, 2), (3, 7, 2), (2, 2, 9), (4, 33, 17), (1, 64, 63)]
    shapes += [(int(rng.integers(1, 5)), int(rng.integers(2, 80)), int(rng.integers(2, 80))) for _ in range(7)]
    for case, (B, H, W) in enumerate(shapes):
        im_ref, im = [rng.uniform(-0.5, 0.5, (B, 3, H, W)).astype(np.float32) for _ in range(2)]
        Cj = int(rng.choice([1, 3]))
        jm_ref, jm = [(rng.random((B, Cj, H, W)) < 0.9).astype(np.float32) for _ in range(2)]
        flows = []
        for _ in range(2):
            f = (rng.standard_normal((B, H, W, 2)) * 1.5).astype(np.float32)
            f[rng.random((B, H, W)) < 0.3] = 0
            integer = rng.random((B, H, W)) < 0.1
            f[integer] = np.round(f[integer])
            f[rng.random((B, H, W)) < 0.03] += 1000.0
            flows.append(f)
        gl = rng.uniform(0.5, 1.5, (B,)).astype(np.float32)
        use_backward = bool(case % 2)
        res = []
        for crit in (PyramidCriterion("l2"), _Composed()):
            f12, f21 = t(flows[0], cuda, True), t(flows[1], cuda, True)
            loss, masks, warps, diffs = imgflowarp.pair_consist([f12, f21], t(im_ref, cuda), t(im, cuda), t(jm_ref, cuda),
                                                                t(jm, cuda), crit, use_backward=use_backward, outputs="full")
            (loss * t(gl, cuda)).sum().backward()
            g12 = n(f12.grad) if f12.grad is not None else np.zeros_like(flows[0])
            res.append((n(loss), g12, n(f21.grad), masks, warps, diffs))
        (lf, g12f, g21f, mf, wf, df), (lc, g12c, g21c, mc, wc, dc) = res
        what = f"case {case} B={B} H={H} W={W} Cj={Cj}"
        close(lf, lc, 1e-5, 1e-7, f"{what}: loss")
        close(g12f, g12c, 1e-4, 1e-7, f"{what}: grad_flow12")
        close(g21f, g21c, 1e-4, 1e-7, f"{what}: grad_flow21")
        for i in (0, 1):
            assert torch.equal(mf[i]["full_mask"], mc[i]["full_mask"]), what
            assert torch.equal(mf[i]["warp_mask"], mc[i]["warp_mask"]), what
            close(n(wf[i]), n(wc[i]), 1e-5, 2e-6, f"{what}: warp")
            close(n(df[i]), n(dc[i]), 1e-5, 2e-6, f"{what}: squared diff")
