"""The frame-pair step on meshes other than synth.random_scene's one: tests/pair_mesh_cases.py's CASES -- the smallest shapes
at which the launchers take each of their mesh-dependent decisions (parts and their hand / object split, boxes in or beyond
LDS, the prologue's LDS opt-in, the V <= 2560 gate from both sides, 16 scatter groups, an odd vertex count, the collate
shape, no object at all) -- through ``opticalflow.flow_pair_loss`` on (hand, object) parts, against a CPU oracle that shares
nothing with the product: W.get_opticalflow + W.pair_consist for flows and losses, and W.pair_consist_grad +
W.get_opticalflow_vertex_grad (float64, pinned to the reference run in tests/test_oracle_warp.py) for the gradient of the
weighted losses with respect to the four vertex tensors, element by element.

Which plan branch a case takes is NOT asserted here: tests/test_pair_mesh_cases_host.py proves that on the CPU for a 256-CU
device, and this file prints the device's compute-unit count.  Inputs live in tests/guarded_alloc.py's guarded storage, render
outputs are poisoned, every case starts from an empty plan cache, and the struct path's second call (another seed, the same
plan, LIST_CLEAN, no poison: the scratch holds the first seed's values) has to give the second seed's oracle results.

Rules.  Flows: the non-zero pattern under the covered tiles equals the oracle's EXACTLY (the precondition of a per-element
gradient comparison; seeds are chosen for it, a mismatch fails), NaN under uncovered tiles, values within 1e-4 x max(|ref|, 1).
Losses (forward, forward + backward, the node's own sum and mean): 2e-5 x max(1, |ref|) (fuzz sweep 8's figures); l2: 1e-5
relative + 1e-7 (test_gpu_l2_criterion.py's against its reference).  Vertex gradients: |got - ref| <= 1e-4 |ref| + 1e-5 x the
largest |ref| of the same sample and leaf (test_gpu_raster.py's rule, normalised per sample instead of per tensor).

Measured.  Oracle seconds: 8 threads, per seed (a fused case runs two), on a slow server CPU -- the MI355X's host took 0.1 to
1.2 s per seed.  Errors: MI355X (256 compute units), the largest over both seeds and every path of the case, in
units of the rule; every flow agreed to better than 0.001 of its rule and every non-zero pattern was exact.  No case exceeded
the gradient rule, so no bound comes from the oracle's fp32 chain (FP32_CHAIN is empty).

    case  oracle s  flows    losses  gradients
    A       0.4     < 0.001  0.001   0.004
    B       2.7     < 0.001  0.002   0.008
    C       3.0     < 0.001  0.002   0.010
    D       6.1     < 0.001  0.002   0.010
    E       1.2     < 0.001  0.001   0.008
    F       3.4     < 0.001  0.001   0.008    (raster 32: 13.3 s at 64)
    G       3.7     < 0.001  0.002   0.009    (raster 32: 14.3 s at 64)
    H       2.8     < 0.001  0.001   0.007
    I       0.6     < 0.001  0.001   0.006    (compact / widened batch: 0.001, 0.005)
    J       1.3     < 0.001  0.001   0.006    (l2: losses 0.010, gradients 0.007)
    K       1.1     < 0.001  0.001   0.006    (composed path, gather fallback)
    L       0.2     < 0.001  0.001   0.005    (composed path, hand only)

F and G run at raster 32, where the jitter borders (up to 16 pixels a side) leave some samples without a valid pixel: their
masked mean divides by 1 and their loss is exactly zero in the oracle and on the device.  The whole file takes 20 s on the GPU.
"""
import time

import numpy as np
import pytest
import torch

from handobjectconsist_amd.utils import synth
from oracle import raster_ref as R
from oracle import warp_ref as W
from tests import guarded_alloc as G
from tests import pair_mesh_cases as P

pytestmark = pytest.mark.gpu

LEAVES = ("hand 1", "object 1", "hand 2", "object 2")
SECOND_SEED = 100  # added to a case's seed for the second call through its plan
WM = 3.0           # weight of the batch mean


def _weights(B):
    """per-sample weights of loss_fwd, loss_bwd and their sum (distinct per sample), as numpy fp32"""
    lin = lambda a, b: np.linspace(a, b, B).astype(np.float32)
    return lin(0.5, 1.5), lin(2.0, 0.25), lin(-0.5, 0.75)


# ---------------------------------------------------------------------------------------------------
# the oracle, once per (case, seed) and (criterion, batch type): shared by the tests, never written to
# ---------------------------------------------------------------------------------------------------
_FORWARD, _ORACLE = {}, {}


def _crop(case):
    Wd, H = case["crop"]
    return Wd, H


def _oracle_forward(name, seed):
    key = (name, seed)
    if key not in _FORWARD:
        case = P.CASES[name]
        s = P.scene_of(case, seed)
        is_ = case["raster"]
        Rm, tm, dm = P.camera(case["B"], case["per_sample_cam"])
        kw = dict(R=Rm, t=tm, dist_coeffs=dm, orig_size=is_, image_size=is_, anti_aliasing=False, near=0.1, far=100, eps=1e-3,
                  num_threads=8, keep_saved=True)
        t0 = time.perf_counter()
        flows, renders, factors = W.get_opticalflow(R, [s["verts1"], s["verts2"]], s["faces"], [s["K1"], s["K2"]], kw, orig_img_size=_crop(case),
                                                    ignore_face_idxs=synth.HAND_IGNORE_FACES, return_renders=True, return_masks=True)
        for f in flows:
            f.setflags(write=False)
        _FORWARD[key] = dict(scene=s, kw=kw, flows=flows, renders=renders, factors=factors, seconds=time.perf_counter() - t0)
    return _FORWARD[key]


def _images(case, seed, compact):
    """(image_ref, image, jitter_ref, jitter) as numpy fp32; ``compact``: the images rounded to bf16 (what the compact batch holds)"""
    Wd, H = _crop(case)
    im_ref, im, jm_ref, jm = synth.random_images(case["B"], H, Wd, seed + 1)
    Cj = case["jitter_channels"]
    jm_ref, jm = np.ascontiguousarray(jm_ref[:, :Cj]), np.ascontiguousarray(jm[:, :Cj])
    if compact:
        im_ref, im = (torch.from_numpy(x).bfloat16().float().numpy() for x in (im_ref, im))
    return im_ref, im, jm_ref, jm


def _oracle(name, seed, crit="l1", compact=False):
    key = (name, seed, crit, compact)
    if key not in _ORACLE:
        case = P.CASES[name]
        fwd = _oracle_forward(name, seed)
        s, B = fwd["scene"], case["B"]
        images = _images(case, seed, compact)
        t0 = time.perf_counter()
        lf, lb = W.pair_consist(fwd["flows"], *images, True, criterion=crit)[4]
        wf, wb, ws = _weights(B)
        # total = sum wf lf + sum wb lb + sum ws (lf + lb) + WM mean(lf + lb)
        cf, cb = wf + ws + np.float32(WM / B), wb + ws + np.float32(WM / B)
        g21 = W.pair_consist_grad(fwd["flows"], *images, cf, False, criterion=crit)[1]
        g12 = W.pair_consist_grad(fwd["flows"], *images, cb, True, criterion=crit)[0]
        args = (R, [s["verts1"], s["verts2"]], s["faces"], [s["K1"], s["K2"]], fwd["kw"], [g12, g21], _crop(case), synth.HAND_IGNORE_FACES)
        gv1, gv2 = W.get_opticalflow_vertex_grad(*args, forward=(fwd["renders"], fwd["factors"]))
        nh = synth.HAND_VERTS
        _ORACLE[key] = dict(lf=lf.astype(np.float64), lb=lb.astype(np.float64), grads=(gv1[:, :nh], gv1[:, nh:], gv2[:, :nh], gv2[:, nh:]),
                            grad_args=args, seconds=fwd["seconds"] + time.perf_counter() - t0)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------
# the device run
# ---------------------------------------------------------------------------------------------------


def _clear_caches():
    from handobjectconsist_amd.neurender import rasterize
    from handobjectconsist_amd.warping import imgflowarp, opticalflow, pairstep

    for cache in (pairstep._PLANS, pairstep._FACES64, opticalflow._FACES2_CACHE, opticalflow._LUT_CACHE, opticalflow._LUT_BY_ID,
                  rasterize._BG_CACHE, imgflowarp._GRID_CACHE):
        cache.clear()


class _Run:
    """one case on the device: guarded inputs, a renderer, the four leaves"""

    def __init__(self, cuda, monkeypatch, name):
        from handobjectconsist_amd.neurender.renderer import Renderer

        self.cuda, self.mp, self.name, self.case = cuda, monkeypatch, name, P.CASES[name]
        _clear_caches()
        self.alloc = G.GuardedAllocator(cuda)
        self.alloc.install(monkeypatch)
        case, is_ = self.case, self.case["raster"]
        Rm, tm, dm = P.camera(case["B"], case["per_sample_cam"])
        self.ren = Renderer(image_size=is_, R=self.up(Rm), t=self.up(tm), K=self.up(np.ones((1, 3, 3), np.float32)), dist_coeffs=self.up(dm),
                            orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True, light_intensity_ambient=0.8)
        cus = torch.cuda.get_device_properties(cuda).multi_processor_count
        print(f"PAIR-MESHES {name}: {cus} compute units" + ("" if cus == 256 else
              " -- NOT 256: the parts coverage tests/test_pair_mesh_cases_host.py proves does not describe this run"))

    def up(self, a, grad=False):
        """a test-made input in guarded storage"""
        with self.alloc.paused():
            x = torch.from_numpy(np.ascontiguousarray(a)).to(self.cuda).clone()
        x = self.alloc.guard(x)
        return x.requires_grad_(True) if grad else x

    def close(self):
        damage = self.alloc.check()
        self.alloc.uninstall()
        _clear_caches()
        assert not damage, "\n".join(damage)

    def batch(self, seed, compact):
        im_ref, im, jm_ref, jm = _images(self.case, seed, False)
        if compact == "widened":
            im_ref, im = (torch.from_numpy(x).bfloat16().float().numpy() for x in (im_ref, im))
        out = [self.up(x) for x in (im_ref, im, jm_ref, jm)]
        if compact is True:
            with self.alloc.paused():
                out = [out[0].bfloat16(), out[1].bfloat16(), out[2].to(torch.uint8), out[3].to(torch.uint8)]
            out = [self.alloc.guard(x) for x in out]
        return out

    def total(self, lf, lb, lsum, mean):
        wf, wb, ws = (self.up(w) for w in _weights(self.case["B"]))
        return (lf * wf).sum() + (lb * wb).sum() + (lsum * ws).sum() + WM * mean

    def fused(self, seed, path, crit_code, compact=False, poison=True):
        """flow_pair_loss on (hand, object) parts: (result or None, leaves)"""
        from handobjectconsist_amd.warping import opticalflow

        self.mp.setattr(opticalflow, "DEBUG_POISON_RENDER_OUTPUTS", poison)
        self.mp.setattr(opticalflow, "USE_PAIR_STEP", path == "step")
        case, s = self.case, _oracle_forward(self.name, seed)["scene"]
        B = case["B"]
        hand_faces = s["hand_faces"][None].repeat(B, 0) if case["hand_batched"] else s["hand_faces"]
        leaves = [self.up(s[k], grad=True) for k in ("hand_verts1", "obj_verts1", "hand_verts2", "obj_verts2")]
        res = opticalflow.flow_pair_loss([(leaves[0], leaves[1]), (leaves[2], leaves[3])], (self.up(hand_faces), self.up(s["obj_faces"])),
                                         [self.up(s["K1"]), self.up(s["K2"])], self.ren, _crop(case), *self.batch(seed, compact),
                                         ignore_face_idxs=synth.HAND_IGNORE_FACES, with_sum=True, with_mean="sum", criterion=crit_code)
        return res, leaves

    def composed(self, seed, crit_name):
        """get_opticalflow + pair_consist on the concatenated mesh: ((lf, lb, flows, lsum, mean), [verts1, verts2])"""
        from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
        from handobjectconsist_amd.warping import imgflowarp, opticalflow

        self.mp.setattr(opticalflow, "DEBUG_POISON_RENDER_OUTPUTS", True)
        case, s = self.case, _oracle_forward(self.name, seed)["scene"]
        v1, v2 = self.up(s["verts1"], grad=True), self.up(s["verts2"], grad=True)
        flows = opticalflow.get_opticalflow([v1, v2], self.up(s["faces"]), [self.up(s["K1"]), self.up(s["K2"])], self.ren, orig_img_size=_crop(case),
                                            ignore_face_idxs=synth.HAND_IGNORE_FACES)
        batch = self.batch(seed, False)
        crit = PyramidCriterion(crit_name)
        both = imgflowarp.pair_consist(flows, *batch, crit, use_backward=True, outputs="loss")[0]
        lf = imgflowarp.pair_consist(flows, *batch, crit, use_backward=False, outputs="loss")[0]
        return (lf, both - lf, flows, both, both.mean()), [v1, v2]


def _units(err, tol):
    """the largest error in units of its tolerance (an error where the tolerance is zero: inf)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(u.max()) if u.size else 0.0


def _check_values(name, what, res, ref_flows, orc, crit, sparse):
    """flows (pattern, uncovered tiles, values) and the four loss outputs against the oracle; prints the figures"""
    lf, lb, flows, lsum, mean = res
    case = P.CASES[name]
    B, is_ = case["B"], case["raster"]
    Wd, H = _crop(case)
    ref = np.concatenate(ref_flows, 0)
    if sparse:
        base = flows[0]._base
        hit = base._hoc_coverage[0]
        words = hit.contiguous().view(torch.int32).view(2 * B, (is_ + 7) // 8, (is_ + 31) // 32).cpu().numpy() != 0
        yy, xx = np.mgrid[0:H, 0:Wd]
        defined = words[:, (is_ - 1 - yy) >> 3, xx >> 5]
        got = base.detach().cpu().numpy()
        assert np.isnan(got[~defined]).all(), f"{what}: something is written under uncovered tiles"
        assert not (ref[~defined] != 0).any(), f"{what}: the oracle has a flow under a tile the render left uncovered"
    else:
        got = np.concatenate([f.detach().cpu().numpy() for f in flows], 0)
        defined = np.ones(got.shape[:3], bool)
    assert tuple(got.shape) == ref.shape
    assert np.isfinite(got[defined]).all(), f"{what}: non-finite flow under a covered tile"
    differ = int(((got != 0) != (ref != 0))[defined].sum())
    assert differ == 0, f"{what}: the flows' non-zero pattern differs from the oracle's at {differ} of {int((ref != 0).sum())} elements"
    assert (ref != 0).any()
    err = np.abs(got - ref)[defined]
    flow_units = _units(err, np.full(err.shape, 1e-4 * max(float(np.abs(ref).max()), 1.0)))
    n = lambda x: x.detach().double().cpu().numpy()
    rf, rb = orc["lf"], orc["lb"]
    pairs = (("loss_fwd", n(lf), rf), ("loss_fwd + loss_bwd", n(lf) + n(lb), rf + rb), ("the node's sum", n(lsum), rf + rb),
             ("the node's mean", n(mean).reshape(1), np.array([(rf + rb).mean()])))
    loss_units = 0.0
    for _, g, r in pairs:
        tol = (1e-5 * np.abs(r) + 1e-7) if crit == "l2" else np.full(r.shape, 2e-5 * max(1.0, float(np.abs(r).max())))
        loss_units = max(loss_units, _units(np.abs(g - r), tol))
    print(f"PAIR-MESHES {what}: flows {flow_units:.3f}, losses {loss_units:.3f} (units of their rules); loss_fwd {rf.mean():.4f} loss_bwd {rb.mean():.4f}")
    assert rf.max() > 0 and rb.max() > 0
    assert flow_units <= 1.0, f"{what}: flow values"
    assert loss_units <= 1.0, f"{what}: losses"


# case -> (fp32 chain's error, bound) in units of the rule, where DESIGN section 2's factor applies (see _check_grads)
FP32_CHAIN = {}


def _check_grads(name, what, grads, orc):
    """each vertex gradient against the float64 oracle: 1e-4 relative + 1e-5 x the largest |gradient| of the same sample and leaf"""
    worst = 0.0
    for got, ref, leaf in zip(grads, orc["grads"], LEAVES):
        if ref.shape[1] == 0:
            assert got is None or got.numel() == 0
            continue
        g = got.detach().double().cpu().numpy()
        assert g.shape == ref.shape and np.isfinite(g).all(), (what, leaf)
        scale = np.abs(ref).max(axis=(1, 2), keepdims=True)
        assert scale.max() > 0, (what, leaf)
        u = _units(np.abs(g - ref), 1e-4 * np.abs(ref) + 1e-5 * scale)
        print(f"PAIR-MESHES {what}: d/d {leaf}: {u:.3f} of the rule (largest |gradient| {scale.max():.3e})")
        worst = max(worst, u)
    bound = 1.0
    if worst > 1.0:
        # the same oracle chain with its existing fp32 pieces (R.backward_textures, fp32 sums) against the float64 chain: what an
        # fp32 evaluation in the reference's order is off by under this rule (printed; a case whose bound it sets is in FP32_CHAIN)
        f32 = W.get_opticalflow_vertex_grad(*orc["grad_args"], fp32=True)
        nh = synth.HAND_VERTS
        chain = 0.0
        for g, ref in zip((f32[0][:, :nh], f32[0][:, nh:], f32[1][:, :nh], f32[1][:, nh:]), orc["grads"]):
            if ref.shape[1]:
                chain = max(chain, _units(np.abs(g.astype(np.float64) - ref), 1e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max(axis=(1, 2), keepdims=True)))
        print(f"PAIR-MESHES {what}: the oracle's fp32 chain is {chain:.3f} of the rule off its float64 chain")
        if name in FP32_CHAIN:
            bound = FP32_CHAIN[name][1]
    assert worst <= bound, f"{what}: vertex gradients at {worst:.3f} of the rule (bound {bound})"


def _crit_code(crit):
    from handobjectconsist_amd import _lib

    return {"l1": _lib.CRITERION_L1, "l2": _lib.CRITERION_L2}[crit]


def _fused_case(cuda, monkeypatch, name, path, crit="l1"):
    from handobjectconsist_amd.warping import pairstep

    case = P.CASES[name]
    run = _Run(cuda, monkeypatch, name)
    try:
        for call, seed in enumerate((case["seed"], case["seed"] + SECOND_SEED)[:2 if path == "step" else 1]):
            what = f"{name} {path} {crit} call {call}"
            orc = _oracle(name, seed, crit)
            print(f"PAIR-MESHES {what}: oracle {orc['seconds']:.1f} s")
            # (the second call: no poison, so that the plan vouches for its list header and the scratch keeps the first seed's values)
            res, leaves = run.fused(seed, path, _crit_code(crit), poison=call == 0)
            assert res is not None, f"{what}: the fused path must take this case"
            lf, lb, flows, lsum, mean = res
            _check_values(name, what, res, _oracle_forward(name, seed)["flows"], orc, crit, sparse=True)
            grads = torch.autograd.grad(run.total(lf, lb, lsum, mean), leaves)
            _check_grads(name, what, grads, orc)
            if path == "step":
                assert len(pairstep._PLANS) == 1, "both calls go through one plan"
                plan = next(iter(pairstep._PLANS.values()))
                assert bool(plan.st.flags & pairstep.LIST_CLEAN) == (call == 1), "the second call runs on the list header the first one left clean"
    finally:
        run.close()


FUSED = [n for n, c in P.CASES.items() if c["fused"]]
NODE = [n for n, c in P.CASES.items() if c["node"]]
assert len(NODE) == 3 and FUSED == list("ABCDEFGHIJ")


@pytest.mark.parametrize("name", FUSED)
def test_pair_step_on_other_meshes(cuda, monkeypatch, name):
    """the struct path (mr_pair_step_forward / _backward), two calls through one plan"""
    _fused_case(cuda, monkeypatch, name, "step")


@pytest.mark.parametrize("name", NODE)
def test_node_pair_on_other_meshes(cuda, monkeypatch, name):
    """the node pair (_FlowVertexStageParts + _FlowPairLossFunction: the prologue as a launch of its own)"""
    _fused_case(cuda, monkeypatch, name, "node")


def test_l2_criterion_on_another_mesh(cuda, monkeypatch):
    _fused_case(cuda, monkeypatch, P.L2_CASE, "step", crit="l2")


def test_compact_batch_on_another_mesh(cuda, monkeypatch):
    """bf16 images and u8 masks as they are: losses, flows and coverage bit for bit those of the widened fp32 batch (as
    test_gpu_compact_batch.py asserts for the one scene), which in turn meets the oracle on the rounded images"""
    name = P.COMPACT_CASE
    case = P.CASES[name]
    run = _Run(cuda, monkeypatch, name)
    try:
        seed = case["seed"]
        orc = _oracle(name, seed, "l1", compact=True)
        out = {}
        for kind in ("widened", True):
            what = f"{name} step l1 {'compact' if kind is True else 'widened'}"
            res, leaves = run.fused(seed, "step", _crit_code("l1"), compact=kind)
            assert res is not None, what
            lf, lb, flows, lsum, mean = res
            _check_values(name, what, res, _oracle_forward(name, seed)["flows"], orc, "l1", sparse=True)
            _check_grads(name, what, torch.autograd.grad(run.total(lf, lb, lsum, mean), leaves), orc)
            base = flows[0]._base
            hit = base._hoc_coverage[0].clone()
            out[kind] = [x.detach().clone() for x in (lf, lb, lsum, mean.reshape(1))] + [torch.nan_to_num(base.detach(), nan=-7.0), hit]
        for x, y, label in zip(out[True], out["widened"], ("loss_fwd", "loss_bwd", "loss_bwd + loss_fwd", "batch mean", "flows", "coverage bytes")):
            assert torch.equal(x, y), label
        assert not torch.equal(run.batch(seed, "widened")[1], run.batch(seed, False)[1]), "the images must actually lose bits in bf16"
    finally:
        run.close()


def _composed_case(cuda, monkeypatch, name):
    case = P.CASES[name]
    run = _Run(cuda, monkeypatch, name)
    try:
        seed = case["seed"]
        what = f"{name} composed l1"
        orc = _oracle(name, seed, "l1")
        print(f"PAIR-MESHES {what}: oracle {orc['seconds']:.1f} s")
        for path in ("step", "node"):
            res, _ = run.fused(seed, path, _crit_code("l1"))
            assert res is None, f"{name}: flow_pair_loss must hand this pair to the composed path ({path})"
        res, (v1, v2) = run.composed(seed, "l1")
        _check_values(name, what, res, _oracle_forward(name, seed)["flows"], orc, "l1", sparse=False)
        g1, g2 = torch.autograd.grad(run.total(res[0], res[1], res[3], res[4]), [v1, v2])
        nh = synth.HAND_VERTS
        _check_grads(name, what, (g1[:, :nh], g1[:, nh:], g2[:, :nh], g2[:, nh:]), orc)
    finally:
        run.close()


def test_composed_path_past_the_vertex_limit(cuda, monkeypatch):
    """V = 2561: flow_pair_loss returns None; get_opticalflow + pair_consist (mr_render_flow_backward answers NOTIMPL, the
    vertex-colour backward takes its gather) meet the same assertions against the same oracle"""
    _composed_case(cuda, monkeypatch, "K")


def test_objectless_pair_takes_the_composed_path(cuda, monkeypatch):
    """no object vertices: pair_step and flow_pair_loss answer None as for every other unsupported shape (they used to raise),
    and the composed path on the hand alone gives the oracle's results"""
    _composed_case(cuda, monkeypatch, "L")
