"""Where the kernels touch memory ("guard bands"): every case runs twice with the same seeds -- on plain
tensors, then under tests/guarded_alloc.py with every test-made input passed through ``guard()`` -- and has to

(a) leave both bands of every guarded allocation as they were filled (no store before or behind an output, a workspace
    or a gradient buffer);
(b) hand the C-ABI no pointer that lies outside a guarded interior or one of the case's declared constants (module
    parameters / buffers, ``layer.hip_constants()["tensors"]``, the grid cache -- and the pinned HOST words the renders
    report their tile-list length to, which the guarded factories pass through like every pinned tensor).  This is the check
    that the guard is not vacuous: a buffer that did not come out of the guarded allocator would go unwatched.  It names
    what the patched factories and ``guard()`` did not make -- the re-homing mode leaves the factory ops' own results, tensors
    made before the allocator was installed or under ``paused()`` and memory torch did not allocate alone -- so a factory
    taken out of the patch list or an input taken out of ``guard()`` turns it red
    (test_a_tensor_outside_the_guard_turns_the_pointer_check_red);
(c) have every compared output in guarded storage;
(d) give the dense outputs and the leaves' gradients of the plain run, bit for bit -- an over-READ that is used shows up
    here, the bands and every unwritten interior being NaN.  Two accumulations are left to float atomics and are compared
    with the tolerance of their own parity tests instead: ``meshreg_post`` backward's per-sample sums
    (test_meshreg_post_hip_matches_torch_ops: 2e-4 relative + 2e-5 of the largest gradient) and the vertex gradients of the
    scatter in ``flow_pair_loss`` (test_scatter_work_lists_equal_the_listing_form: 1e-5 relative + 2e-6 of the largest).
    (The cases this module adds to the listed ones bring a third: the gradient to the face coordinates of the generic render,
    see RASTER_TOL.)

``grad_x`` of ``warp`` is a float-atomics sum as well (``mr_warp_backward`` scatters ``g * weight`` to the four taps, as torch's
``grid_sample`` backward does); the order of arrival matters only where a partial sum ROUNDS, so the warp cases draw operands
for which none does -- sample positions on a lattice of eighths of a pixel, gradients in eighths (``_exact_warp_operands``, the
way tests/test_gpu_trunk_exact.py makes the trunk's channel sums exact) -- and stay bit for bit.

The cases are the smallest shapes at which the edges exist: rasters that are no multiple of the 32 x 8 tile, widths that
are no multiple of a 16-byte store, one element past a 256-thread grid, odd byte counts, empty face lists."""
import json
import os
import types

import numpy as np
import pytest
import torch

from handobjectconsist_amd.utils import synth
from tests import guarded_alloc as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
POST_TOL = (2e-4, 2e-5)      # meshreg_post backward (float atomics): rtol, atol as a share of the largest |gradient|
SCATTER_TOL = (1e-5, 2e-6)   # the scatter of flow_pair_loss (float atomics)
# Cases this module adds to the listed ones, for the kernels behind the gradient to the FACE COORDINATES of the generic render
# (mr_render_backward's kernel D and its workspace; RasterizeFunction's five upstream-compatible entry points, which
# tests/test_gpu_strided_inputs.py needs a caller for): those sums are float atomics too, as upstream's are, and are compared
# with the tolerance of test_fused_backward_matches_oracle / test_compat_five_entry_points_match_oracle
RASTER_TOL = (1e-4, 1e-5)

CASES = {}


def case(name, *args, **kw):
    def register(fn):
        assert name not in CASES
        CASES[name] = (fn, args, kw)
        return fn
    return register


class Ctx:
    """what a case needs: the device, ``ctx(x)`` = a test-made input on the device (guarded in the guarded run), monkeypatch"""

    def __init__(self, dev, alloc, monkeypatch, unguarded=None):
        """``unguarded``: the index of ONE ``ctx(...)`` call whose tensor is left out of ``guard()`` (the pointer check's
        self-test)"""
        self.dev, self.alloc, self.mp, self.unguarded, self.made = dev, alloc, monkeypatch, unguarded, 0

    def __call__(self, a, grad=False, kind=None):
        """(``kind``: the view tests/test_gpu_strided_inputs.py has to make of this operand, where the case depends on it)"""
        if a is None:
            return None
        x = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if self.alloc is None:
            x = x.detach().to(self.dev)
        else:
            with self.alloc.paused():  # the upload is plain memory: only guard() brings the input into guarded storage
                x = x.detach().to(self.dev).clone()
            if self.made != self.unguarded:
                x = self.alloc.guard(x)
        self.made += 1
        return x.requires_grad_(True) if grad else x

    def backward(self, outs, grads):
        """the case's backward pass: ``grads`` are test-made inputs (``ctx(...)``), one per output"""
        torch.autograd.backward(list(outs), list(grads))

    def host(self, a):
        """a test-made HOST array, as it is"""
        return a

    def camera(self, x, B):
        """a batch-1 camera tensor (K, R [1,3,3], t [1,3], dist_coeffs [1,5]) for a batch of ``B``"""
        return self(x)


def module_constants(*modules):
    out = []
    for m in modules:
        out += list(m.parameters()) + list(m.buffers())
        if hasattr(m, "hip_constants"):
            out += [t for t in m.hip_constants()["tensors"] if t is not None]
    return out


def _rand(g, *shape, s=1.0):
    return s * torch.randn(*shape, generator=g)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) % 2 ** 31)


# ------------------------------------------------------------------------------------------------------------ renders
def _renderer(ctx, is_, B, aa=False):
    from handobjectconsist_amd.neurender.renderer import Renderer

    return Renderer(image_size=is_, R=ctx.camera(torch.eye(3)[None], B), t=ctx.camera(torch.zeros(1, 3), B), K=ctx.camera(torch.ones(1, 3, 3), B),
                    dist_coeffs=ctx.camera(torch.zeros(1, 5), B), orig_size=is_, anti_aliasing=aa, fill_back=True, near=0.1, no_light=True,
                    light_intensity_ambient=0.8)


@case("render_generic-raster5", 5)
@case("render_generic-raster40", 40)
@case("render_generic-raster40-aa", 40, aa=True)
@case("render_generic-raster40-no_faces", 40, empty=True)
@case("render_generic-raster5-face_gradients", 5, face_grads=True)
@case("render_generic-raster40-face_gradients", 40, face_grads=True)
@case("render_generic-raster40-five_entry_points", 40, fused=False, face_grads=True)
# (B = 3, F = 5 on rasters of 2 and 6 pixels: the strip weights of mr_render_backward's workspace -- 2 B is / L words, cleared by
# the marking launch one word per thread -- outnumber that launch's pixel quads, and every region is smaller than its slot)
@case("render_generic-raster2-5_faces-face_gradients", 2, face_grads=True, few=True)
@case("render_generic-raster6-5_faces-face_gradients", 6, face_grads=True, few=True)
def render_generic(ctx, is_, aa=False, empty=False, fused=True, face_grads=False, few=False):
    """rasterize_rgbad on textures, rgb / alpha / depth, forward + backward to the textures (the training setting: a fixed-order
    gather, bit-reproducible); ``face_grads``: to the face coordinates as well (float atomics); ``fused=False``:
    RasterizeFunction on the five upstream-compatible entry points; ``few``: five large random triangles of both windings"""
    from handobjectconsist_amd.neurender import rasterize
    from tests.test_gpu_raster import projected_faces

    ctx.mp.setattr(rasterize, "USE_FUSED", fused)
    B = 3
    faces, tex = projected_faces(B, is_, 7)
    if empty:
        faces, tex = faces[:, :0], tex[:, :0]
    if few:
        rng = np.random.default_rng(is_)
        faces = rng.uniform(-1.3, 1.3, (B, 5, 3, 3)).astype(np.float32)
        faces[..., 2] = rng.uniform(0.3, 3.0, (B, 5, 3))
        faces[:, 1::2] = faces[:, 1::2, ::-1]
        tex = rng.uniform(-1, 1, (B, 5, 2, 2, 2, 3)).astype(np.float32)
    f, x = ctx(faces, grad=face_grads), ctx(tex, grad=True)
    out = rasterize.rasterize_rgbad(f, x, is_, aa, 0.1, 100, 1e-3, (0.1, 0.2, 0.3))
    g = _gen(is_, aa, empty)
    grads = [ctx(_rand(g, *out[k].shape)) for k in ("rgb", "alpha", "depth")]
    ctx.backward([out["rgb"], out["alpha"], out["depth"]], grads)
    return dict(out=dict(rgb=out["rgb"], alpha=out["alpha"], depth=out["depth"], grad_faces=f.grad, grad_textures=x.grad),
                loose=dict(grad_faces=RASTER_TOL, **({} if fused else dict(grad_textures=RASTER_TOL))),
                wants_call=("mr_render_backward",) if few else ())


@case("render_vertex_colours-raster40", 40)
def render_vertex_colours(ctx, is_):
    B = 3
    s = synth.random_scene(B, seed=31, image_size=is_)
    cols = np.random.default_rng(5).uniform(-3, 3, (B, s["verts1"].shape[1], 3)).astype(np.float32)
    ren = _renderer(ctx, is_, B)
    c = ctx(cols, grad=True)
    out = ren.render_vertex_colors(ctx(s["verts1"]), ctx(s["faces"]), c, K=ctx(s["K1"]))
    ctx.backward([out["rgb"]], [ctx(_rand(_gen(is_), *out["rgb"].shape))])
    return dict(out=dict(rgb=out["rgb"], alpha=out["alpha"], depth=out["depth"], grad_colours=c.grad))


# ------------------------------------------------------------------------------------------------------- the flow path
def _images(ctx, B, H, W, Cj, seed, compact=False):
    im_ref, im, jm_ref, jm = (torch.from_numpy(np.ascontiguousarray(a)) for a in synth.random_images(B, H, W, seed))
    jm_ref, jm = jm_ref[:, :Cj].contiguous(), jm[:, :Cj].contiguous()
    if compact:
        im_ref, im, jm_ref, jm = im_ref.bfloat16(), im.bfloat16(), jm_ref.to(U8), jm.to(U8)
    return [ctx(x) for x in (im_ref, im, jm_ref, jm)]


@case("opticalflow_then_pair_consist-3x104-56x100-cj1", 3, 104, 56, 100, 1)
@case("opticalflow_then_pair_consist-1x40-27x33-cj3", 1, 40, 27, 33, 3)
# (the two other epilogues of get_opticalflow: one render per frame + _FlowFinalize; a raster that is no multiple of 4 -> the
# flow-mode render + _FlowFinalizeStacked)
@case("opticalflow_then_pair_consist-detach_textures-2x40-27x33-cj3", 2, 40, 27, 33, 3, detach_textures=True)
@case("opticalflow_then_pair_consist-raster42-2x42-27x33-cj1", 2, 42, 27, 33, 1)
def opticalflow_then_pair_consist(ctx, B, is_, H, W, Cj, detach_textures=False):
    """get_opticalflow (stacked flow render, tile list, sparse tiles, pixel records) -> pair_consist(outputs="loss") ->
    backward to the vertices of both frames; the flows under uncovered tiles are not compared (sparse contract)"""
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp, opticalflow

    s = synth.random_scene(B, seed=21, image_size=is_)
    ren = _renderer(ctx, is_, B)
    v1, v2 = ctx(s["verts1"], grad=True), ctx(s["verts2"], grad=True)
    flows = opticalflow.get_opticalflow([v1, v2], ctx(s["faces"]), [ctx(s["K1"]), ctx(s["K2"])], ren, orig_img_size=(W, H),
                                        detach_textures=detach_textures, detach_renders=True, ignore_face_idxs=synth.HAND_IGNORE_FACES,
                                        sparse_flows=True)
    im_ref, im, jm_ref, jm = _images(ctx, B, H, W, Cj, 3)
    loss = imgflowarp.pair_consist(flows, im_ref, im, jm_ref, jm, PyramidCriterion("l1"), use_backward=True, outputs="loss")[0]
    ctx.backward([loss], [ctx(torch.linspace(0.5, 1.5, B))])
    if detach_textures:  # one render per frame + _FlowFinalize
        wants = ("mr_render_vc_forward", "mr_flow_finalize_forward", "mr_flow_finalize_backward")
    elif is_ % 4:  # RasterizeFlowFunction + _FlowFinalizeStacked
        wants = ("mr_render_flow_forward", "mr_occlusion_mask", "mr_flow_finalize_forward", "mr_flow_finalize_backward")
    else:  # _StackedFlowFunction
        wants = ("mr_render_flow_forward", "mr_render_flow_backward")
    return dict(out=dict(loss=loss, grad_verts1=v1.grad, grad_verts2=v2.grad), const=list(imgflowarp._GRID_CACHE.values()),
                wants_call=wants)


def _pair_loss_cases():
    for path in ("nodes", "step"):
        for batch in ("fp32", "compact"):
            for dims in ((2, 72, 72, 72, 1), (3, 104, 56, 100, 3)):
                name = "flow_pair_loss-%s-%s-%dx%d-%dx%d-cj%d" % ((path, batch) + dims)
                case(name, path, batch, *dims)(flow_pair_loss)
        # (B = 1 on a raster of 36: 2 x 5 tiles, every region of the listed pair loss's workspace -- partial | tile_max -- and of
        # the pair step's two buffers ends off the 256-byte grid)
        case("flow_pair_loss-%s-fp32-1x36-33x35-cj1" % path, path, "fp32", 1, 36, 33, 35, 1)(flow_pair_loss)


def flow_pair_loss(ctx, path, batch, B, is_, H, W, Cj):
    """flow_pair_loss on (hand, object) parts: the node pair (_FlowVertexStageParts + _FlowPairLossFunction) and the struct
    calls mr_pair_step_*; fp32 batch and compact batch (bf16 images, u8 masks)"""
    from handobjectconsist_amd.warping import opticalflow

    ctx.mp.setattr(opticalflow, "USE_PAIR_STEP", path == "step")
    s = synth.random_scene(B, seed=31, image_size=is_)
    ren = _renderer(ctx, is_, B)
    leaves = [ctx(s[k], grad=True) for k in ("hand_verts1", "obj_verts1", "hand_verts2", "obj_verts2")]
    hand_faces = ctx(s["hand_faces"].astype(np.int64))
    obj_faces = ctx(s["obj_faces"].astype(np.int64)[None].repeat(B, 0))
    im_ref, im, jm_ref, jm = _images(ctx, B, H, W, Cj, 9, compact=batch == "compact")
    res = opticalflow.flow_pair_loss([(leaves[0], leaves[1]), (leaves[2], leaves[3])], (hand_faces, obj_faces),
                                     [ctx(s["K1"]), ctx(s["K2"])], ren, (W, H), im_ref, im, jm_ref, jm,
                                     ignore_face_idxs=synth.HAND_IGNORE_FACES)
    assert res is not None, "the fused pair node does not apply"
    lf, lb, _flows = res
    ctx.backward([lf, lb], [ctx(torch.linspace(0.5, 1.5, B)), ctx(torch.linspace(2.0, 0.25, B))])
    names = ("grad_hand1", "grad_obj1", "grad_hand2", "grad_obj2")
    out = dict(loss_fwd=lf, loss_bwd=lb, **{n: x.grad for n, x in zip(names, leaves)})
    return dict(out=out, loose={n: SCATTER_TOL for n in names}, wants_call=("mr_pair_step_forward", "mr_pair_step_backward") if path == "step" else
                ("mr_flow_pair_prologue_parts", "mr_flow_pair_backward_unit_tiles"))


_pair_loss_cases()


@case("warp-bilinear-2x3x7x5", "bilinear", (2, 3, 7, 5))
@case("warp-bilinear-1x1x3x2", "bilinear", (1, 1, 3, 2))
@case("warp-nearest-2x3x7x5", "nearest", (2, 3, 7, 5))
@case("warp-nearest-1x1x3x2", "nearest", (1, 1, 3, 2))
def warp(ctx, mode, shape):
    from handobjectconsist_amd.warping import imgflowarp

    g = _gen(*shape)
    B, C, H, W = shape
    flow, grad_out = _exact_warp_operands(g, shape)
    x, flow = ctx(_rand(g, *shape), grad=True), ctx(flow, grad=True)
    out, mask = imgflowarp.warp(x, flow, mode=mode)
    ctx.backward([out], [ctx(grad_out)])
    assert torch.equal(x.grad * 4096, torch.round(x.grad * 4096)), "grad_x is no sum of exact terms: the operands are not exact"
    return dict(out=dict(out=out, mask=mask, grad_x=x.grad, grad_flow=flow.grad))


def _exact_warp_operands(g, shape):
    """(flow, grad_out) for which every partial sum of ``grad_x`` is exact in fp32, whatever order the float atomics arrive in.
    mr_warp_backward samples at ix = ((2 (x + u) / (W - 1) - 1 + 1) W - 1) / 2: with x + u = m (W - 1) / 8 for an integer m the
    division gives m / 4 exactly (no rounding anywhere: small dyadic values, correctly rounded division), so ix = m W / 8 - 1 / 2
    is a multiple of 1/8, and likewise iy; the four weights are then multiples of 1/64.  Gradients in eighths, |g| <= 4: every
    term is a multiple of 2^-9 below 4, a plane has at most 4 H W <= 140 of them, so every sum is a multiple of 2^-9 below 2^10
    -- 19 bits.  m from -4 to 12: positions from half a plane before the first pixel to half a plane behind the last, in and
    out of bounds on every side, every fractional part in eighths."""
    B, C, H, W = shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gx = torch.randint(-4, 13, (B, H, W), generator=g).float() * (max(W - 1, 1) / 8)
    gy = torch.randint(-4, 13, (B, H, W), generator=g).float() * (max(H - 1, 1) / 8)
    flow = torch.stack([gx - xs, gy - ys], 1)
    grad_out = torch.randint(-32, 33, shape, generator=g).float() / 8
    return flow, grad_out


@case("occlusion_mask-2x7x5", (2, 7, 5))
@case("occlusion_mask-1x3x2", (1, 3, 2))
def occlusion_mask(ctx, shape):
    from handobjectconsist_amd.warping import imgflowarp

    g = _gen(*shape)
    B, H, W = shape
    m1, m2 = ((torch.rand(B, 1, H, W, generator=g) < 0.7).float() for _ in range(2))
    f12, f21 = _rand(g, B, 2, H, W, s=1.5), _rand(g, B, 2, H, W, s=1.5)
    o1, o2 = imgflowarp.get_occlusion_mask(ctx(m1), ctx(m2), ctx(f12), ctx(f21))
    return dict(out=dict(occl1=o1, occl2=o2))


@case("pair_consist_dense-2x27x33")
def pair_consist_dense(ctx):
    """the dense pair kernels with the per-pixel debug outputs (masks, warps, diffs)"""
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    B, H, W = 2, 27, 33
    g = _gen(B, H, W)
    keep = lambda: (torch.rand(B, H, W, 1, generator=g) < 0.6).float()
    f12, f21 = ctx(_rand(g, B, H, W, 2, s=2.0) * keep(), grad=True), ctx(_rand(g, B, H, W, 2, s=2.0) * keep(), grad=True)
    im_ref, im, jm_ref, jm = _images(ctx, B, H, W, 3, 4)
    loss, masks, warps, diffs = imgflowarp.pair_consist([f12, f21], im_ref, im, jm_ref, jm, PyramidCriterion("l1"),
                                                        use_backward=True, outputs="full")
    ctx.backward([loss], [ctx(torch.linspace(0.5, 1.5, B))])
    out = dict(loss=loss, grad_flow12=f12.grad, grad_flow21=f21.grad, warp1=warps[0], warp2=warps[1], diff1=diffs[0], diff2=diffs[1])
    for k, m in enumerate(masks):
        out.update({f"warp_mask{k}": m["warp_mask"], f"full_mask{k}": m["full_mask"]})
    return dict(out=out, const=list(imgflowarp._GRID_CACHE.values()))


def _camera(ctx, B, per_sample=False):
    nb = B if per_sample else 1
    ang = torch.linspace(-0.05, 0.05, nb)
    R = torch.eye(3).repeat(nb, 1, 1)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1] = torch.cos(ang), -torch.sin(ang), torch.sin(ang), torch.cos(ang)
    t = torch.linspace(-0.01, 0.01, nb)[:, None].repeat(1, 3)
    dist = torch.linspace(-0.02, 0.02, nb)[:, None] * torch.tensor([1.0, 0.5, 0.1, -0.1, 0.2])
    if per_sample:
        return ctx(R), ctx(t), ctx(dist)
    return ctx.camera(R, B), ctx.camera(t, B), ctx.camera(dist, B)


def _verts(g, B, V):
    v = _rand(g, B, V, 3, s=0.05)
    v[..., 2] += 0.5
    return v


def _intrinsics(g, B, is_):
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 350.0 * is_ / 256 + _rand(g, B, s=5.0)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = is_ / 2 + 1.5, is_ / 2 - 2.5, 1.0
    return K


@case("flow_vertex_stage-V257")
def flow_vertex_stage(ctx):
    from handobjectconsist_amd.warping.opticalflow import _FlowVertexStage

    B, V, is_ = 2, 257, 64
    g = _gen(B, V)
    v1, v2 = ctx(_verts(g, B, V), grad=True), ctx(_verts(g, B, V), grad=True)
    ndc, cols = _FlowVertexStage.apply(v1, v2, ctx(_intrinsics(g, B, is_)), ctx(_intrinsics(g, B, is_)), *_camera(ctx, B, True), is_)
    ctx.backward([cols], [ctx(_rand(g, 2 * B, V, 3))])
    return dict(out=dict(ndc=ndc, cols=cols, grad_verts1=v1.grad, grad_verts2=v2.grad))


def _parts(ctx, g, B, Va, Vb, want):
    return [ctx(_verts(g, B, V), grad=w) for V, w in zip((Va, Vb, Va, Vb), want)]


@case("flow_vertex_stage_parts-Va255-Vb3")
def flow_vertex_stage_parts(ctx):
    """gradients wanted for the object parts only"""
    from handobjectconsist_amd.warping.opticalflow import _FlowVertexStageParts

    B, Va, Vb, is_ = 2, 255, 3, 64
    g = _gen(B, Va, Vb)
    parts = _parts(ctx, g, B, Va, Vb, (False, True, False, True))
    ndc, cols = _FlowVertexStageParts.apply(*parts, ctx(_intrinsics(g, B, is_)), ctx(_intrinsics(g, B, is_)), *_camera(ctx, B), is_)
    ctx.backward([cols], [ctx(_rand(g, 2 * B, Va + Vb, 3))])
    assert parts[0].grad is None and parts[2].grad is None
    return dict(out=dict(ndc=ndc, cols=cols, grad_obj1=parts[1].grad, grad_obj2=parts[3].grad))


def _pair_faces(ctx, g, B, Va, Vb, batched, Fh=5, Fo=3):
    hf = torch.randint(0, Va, (B, Fh, 3) if batched else (Fh, 3), generator=g)
    of = torch.randint(0, Vb, (B, Fo, 3), generator=g)
    return ctx(hf), ctx(of)


@case("flow_pair_prologue_parts-batched_hand_faces", True)
@case("flow_pair_prologue_parts-shared_hand_faces", False)
def flow_pair_prologue_parts(ctx, batched):
    """_FlowVertexStageParts with faces (mr_flow_pair_prologue_parts) and a clear16 region taken from mr_render_clear_bytes"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping.opticalflow import _FlowVertexStageParts

    B, Va, Vb, is_, Fh, Fo = 2, 255, 3, 40, 5, 3
    g = _gen(B, Va, Vb, batched)
    parts = _parts(ctx, g, B, Va, Vb, (True, True, True, True))
    hf, of = _pair_faces(ctx, g, B, Va, Vb, batched)
    F = 2 * (Fh + Fo)  # fill_back
    wbytes = int(_lib.load().mr_render_workspace_bytes(2 * B, F, is_))
    work = torch.full((max(wbytes, 8),), 0xA5, dtype=U8, device=ctx.dev)
    where = _lib.tile_list(work, 2 * B, F, is_)
    assert where is not None, "this raster builds no tile list"
    nclear = int(_lib.load().mr_render_clear_bytes(2 * B, F, is_))
    lo = where[0].value - work.data_ptr()
    assert 0 <= lo and lo + nclear <= work.numel() and nclear > 0
    ndc, cols, faces2 = _FlowVertexStageParts.apply(*parts, ctx(_intrinsics(g, B, is_)), ctx(_intrinsics(g, B, is_)), *_camera(ctx, B), is_,
                                                    hf, of, (where[0], nclear))
    ctx.backward([cols], [ctx(_rand(g, 2 * B, Va + Vb, 3))])
    out = dict(ndc=ndc, cols=cols, faces2=faces2, workspace=work, **{f"grad_part{k}": p.grad for k, p in enumerate(parts)})
    assert bool((work[lo:lo + nclear] == 0).all()), "the clear16 region is not cleared"
    assert bool((work[:lo] == 0xA5).all()) and bool((work[lo + nclear:] == 0xA5).all()), "cleared outside the clear16 region"
    return dict(out=out)


@case("stack_pair_faces-batched_hand_faces", True)
@case("stack_pair_faces-shared_hand_faces", False)
def stack_pair_faces(ctx, batched):
    from handobjectconsist_amd.warping import opticalflow

    B, Va, Vb = 2, 255, 3
    g = _gen(B, Va, Vb, batched)
    hf, of = _pair_faces(ctx, g, B, Va, Vb, batched)
    return dict(out=dict(faces2=opticalflow._stack_pair_faces(hf, of, Va)))


# --------------------------------------------------------------------------------------------------------- MANO, heads
def _mano(ctx, **kw):
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(ncomps=15, **kw).to(ctx.dev)
    layer.hip_constants()
    return layer


@case("mano_pca-B1", 1)
@case("mano_pca-B33", 33)
def mano_pca(ctx, B):
    layer = _mano(ctx, use_pca=True, center_idx=9)
    g = _gen(B, 18)
    p, b = ctx(_rand(g, B, 18, s=0.4), grad=True), ctx(_rand(g, B, 10), grad=True)
    v, j = layer(p, b)
    ctx.backward([v, j], [ctx(_rand(g, B, 778, 3)), ctx(_rand(g, B, 21, 3))])
    return dict(out=dict(verts=v, joints=j, grad_pose=p.grad, grad_betas=b.grad), const=module_constants(layer))


@case("mano_forward_full-pca", True)
@case("mano_forward_full-axisang", False)
# (the padded batch of the backward's split-K partials is 32 at B = 1 and 64 at B = 33; tflag sits behind them)
@case("mano_forward_full-axisang-B1", False, 1)
@case("mano_forward_full-axisang-B33", False, 33)
def mano_forward_full(ctx, use_pca, B=2):
    layer = _mano(ctx, use_pca=use_pca, flat_hand_mean=not use_pca, center_idx=9 if use_pca else None)
    g = _gen(B, use_pca)
    p, b = ctx(_rand(g, B, 18 if use_pca else 48, s=0.4), grad=True), ctx(_rand(g, B, 10), grad=True)
    tr = ctx(_rand(g, B, 3, s=0.1), grad=True)
    v, j = layer.forward_full(p, b, tr)
    ctx.backward([v, j], [ctx(_rand(g, B, 778, 3)), ctx(_rand(g, B, 21, 3))])
    return dict(out=dict(verts=v, joints=j, grad_pose=p.grad, grad_betas=b.grad, grad_trans=tr.grad), const=module_constants(layer))


@case("hand_verts_batch")
def hand_verts_batch(ctx):
    from handobjectconsist_amd.datasets import manogt

    layer = _mano(ctx, use_pca=False, flat_hand_mean=True, center_idx=None)
    n, rng = 3, np.random.default_rng(3)
    fullpose = np.concatenate([rng.standard_normal((n, 3)) * 0.8, rng.standard_normal((n, 45)) * 0.3], 1).astype(np.float32)
    shape = rng.standard_normal((n, 10)).astype(np.float32)
    trans = (rng.standard_normal((n, 3)) * 0.2 + [0, 0, 0.6]).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, n)
    rot = np.stack([np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) for a in ang]).astype(np.float32)
    center = (rng.standard_normal((n, 3)) * 0.1 + [0, 0, 0.6]).astype(np.float32)
    got = manogt.hand_verts_batch(layer, ctx.host(fullpose), ctx.host(shape), ctx.host(trans), device=ctx.dev, flip=np.arange(n) % 2 == 1,
                                  rot_mat=ctx.host(rot), center3d=ctx.host(center))
    return dict(out=dict(verts=got), const=module_constants(layer))


@case("post_heads-Vo1", 1)
@case("post_heads-Vo1025", 1025)
def post_heads(ctx, Vo):
    """mr_meshreg_post_*: the output subset (2, 4) used"""
    from handobjectconsist_amd.models import synthnet

    B = 2
    layer = _mano(ctx, use_pca=True, center_idx=9)
    model = types.SimpleNamespace(mano_layer=layer, obj_trans_factor=100, obj_scale_factor=0.0001)
    g = _gen(B, Vo)
    so = _rand(g, B, 6)
    so[0, 3:] = 0
    K = torch.tensor([[350.0, 0.0, 120.0], [0.0, 350.0, 131.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    K[:, 0, 0] += _rand(g, B, s=20.0)
    K[:, 1, 1] = K[:, 0, 0]
    leaves = [ctx(x, grad=True) for x in (_rand(g, B, 18, s=0.3), _rand(g, B, 10), _rand(g, B, 3), so)]
    o = synthnet.SynthMeshRegNet.post_heads(model, *leaves, ctx(K), ctx(_rand(g, B, Vo, 3, s=0.05)), input_res=(256, 240))
    ctx.backward([o[2], o[4]], [ctx(_rand(g, *o[2].shape)), ctx(_rand(g, *o[4].shape))])
    names = ("grad_pose", "grad_shape", "grad_scaletrans", "grad_st_obj")
    out = dict(zip(("handverts3d", "joints3d", "joints2d", "objverts3d", "objverts2d"), o), **{n: x.grad for n, x in zip(names, leaves)})
    return dict(out=out, loose={n: POST_TOL for n in names}, const=module_constants(layer))


# ------------------------------------------------------------------------------------------------------ the trunk glue
def _bn(ctx, C, g):
    bn = torch.nn.BatchNorm2d(C).to(ctx.dev).eval()
    with torch.no_grad():
        bn.weight.copy_(_rand(g, C, s=0.5) + 1.0)
        bn.weight[0] = -0.7
        bn.bias.copy_(_rand(g, C, s=0.3))
        bn.running_mean.copy_(_rand(g, C, s=0.4))
        bn.running_var.copy_(torch.rand(C, generator=g) * 2 + 0.05)
    return bn


def _act(ctx, g, shape, dtype, cl, grad=False, kind=None):
    x = _rand(g, *shape).to(dtype)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    return ctx(x, grad=grad, kind=kind)


def _pooled(shape):
    N, C, H, W = shape
    return (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


def _glue_cases():
    for dt, dn in ((FP32, "fp32"), (BF16, "bf16")):
        case(f"bn_act-nchw-3x5x17x31-{dn}", (3, 5, 17, 31), dt, False)(bn_act)
        case(f"bn_act-channels_last-2x8x3x5-{dn}", (2, 8, 3, 5), dt, True)(bn_act)
        case(f"block_tail-2x8x3x5-{dn}", (2, 8, 3, 5), dt)(block_tail)
        for shape, cl in (((3, 5, 17, 31), False), ((2, 4, 1, 1), False), ((3, 8, 17, 31), True), ((1, 128, 2, 3), True)):
            name = "x".join(map(str, shape))
            case(f"stem_pool-layout{2 if cl else 0}-{name}-{dn}", shape, dt, cl)(stem_pool)
            if cl:
                case(f"stem_pool-layout1-{name}-{dn}", shape, dt)(stem_pool_layout1)


def bn_act(ctx, shape, dtype, cl):
    """with residual and parameter gradients"""
    from handobjectconsist_amd.nn import frozen_bn

    g = _gen(*shape, cl)
    bn = _bn(ctx, shape[1], g)
    x, r = _act(ctx, g, shape, dtype, cl, True), _act(ctx, g, shape, dtype, cl, True)
    y = frozen_bn.bn_act(x, bn, residual=r, relu=True)
    ctx.backward([y], [_act(ctx, g, shape, dtype, cl)])
    return dict(out=dict(y=y, grad_x=x.grad, grad_residual=r.grad, grad_weight=bn.weight.grad, grad_bias=bn.bias.grad),
                const=module_constants(bn))


def block_tail(ctx, shape, dtype):
    """relu(bn(x) + bn_d(xd)) on channels-last activations, two gradients"""
    from handobjectconsist_amd.nn import frozen_bn

    g = _gen(*shape, 7)
    bn, bn_d = _bn(ctx, shape[1], g), _bn(ctx, shape[1], g)
    # (as views, both stay channels-last -- one element into a flat buffer, misaligned --: any other layout runs as two bn_act
    # calls, which the bn_act cases cover)
    x, xd = _act(ctx, g, shape, dtype, True, True, kind="offset"), _act(ctx, g, shape, dtype, True, True, kind="offset")
    y1, y2 = frozen_bn.bn_add_bn_act(x, bn, xd, bn_d, dup=True)
    ctx.backward([y1, y2], [_act(ctx, g, shape, dtype, True), _act(ctx, g, shape, dtype, True)])
    return dict(out=dict(y=y1, grad_x=x.grad, grad_xd=xd.grad, grad_weight=bn.weight.grad, grad_bias=bn.bias.grad,
                         grad_weight_d=bn_d.weight.grad, grad_bias_d=bn_d.bias.grad), const=module_constants(bn, bn_d),
                wants_call=("mr_bn_add_bn_act_forward", "mr_bn_add_bn_act_backward"))


def stem_pool(ctx, shape, dtype, cl):
    """layout 0 (NCHW) and layout 2 (channels-last, pooled records) through stem_pool, parameter gradients, second gradient"""
    from handobjectconsist_amd.nn import frozen_bn

    g = _gen(*shape, cl, 3)
    bn = _bn(ctx, shape[1], g)
    x = _act(ctx, g, shape, dtype, cl, True)
    y1, y2 = frozen_bn.stem_pool(x, bn, dup=True)
    ctx.backward([y1, y2], [_act(ctx, g, _pooled(shape), dtype, cl), _act(ctx, g, _pooled(shape), dtype, cl)])
    return dict(out=dict(y=y1, grad_x=x.grad, grad_weight=bn.weight.grad, grad_bias=bn.bias.grad), const=module_constants(bn))


def stem_pool_layout1(ctx, shape, dtype):
    """layout 1 (channels-last, arg-max codes, x read by the backward) has no Python caller: the entry points, on buffers
    from the factories"""
    from handobjectconsist_amd import _lib

    g = _gen(*shape, 11)
    N, C, H, W = shape
    P, st = _lib.ptr, _lib.stream_ptr(ctx.dev)
    code = 0 if dtype == FP32 else 1
    w, b, m = ctx(_rand(g, C, s=0.5) + 1.0), ctx(_rand(g, C, s=0.3)), ctx(_rand(g, C, s=0.4))
    v = ctx(torch.rand(C, generator=g) * 2 + 0.05)
    x = _act(ctx, g, shape, dtype, True)
    gy, gy2 = _act(ctx, g, _pooled(shape), dtype, True), _act(ctx, g, _pooled(shape), dtype, True)
    y = torch.empty(_pooled(shape), dtype=dtype, device=ctx.dev, memory_format=torch.channels_last)
    codes = torch.empty((y.numel(),), dtype=U8, device=ctx.dev)
    _lib.call("mr_stem_pool_forward", P(x), P(w), P(b), P(m), P(v), 1e-5, code, 1, P(y), P(codes), N, C, H, W, st)
    gx = torch.empty_like(x)
    gw, gb = torch.empty_like(w), torch.empty_like(b)
    wbytes = int(_lib.load().mr_stem_pool_backward_workspace_bytes(N, C, H, W))
    work = torch.empty((max(wbytes, 1),), dtype=U8, device=ctx.dev)
    _lib.call("mr_stem_pool_backward", P(gy), P(gy2), P(x), P(codes), P(w), P(b), P(m), P(v), 1e-5, code, 1, P(gx), P(gw), P(gb),
              P(work), wbytes, N, C, H, W, st)
    return dict(out=dict(y=y, codes=codes, grad_x=gx, grad_weight=gw, grad_bias=gb))


_glue_cases()


# --------------------------------------------------------------------------------------------------------- the data path
def _frames_cases():
    for (W, H) in ((5, 3), (7, 1)):
        for kind, idt, mdt in (("fp32", FP32, FP32), ("compact", BF16, U8)):
            for mc in (1, 3):
                case(f"frames_to_batch-{W}x{H}-{kind}-mask_channels{mc}", (W, H), idt, mdt, mc)(frames_to_batch)


def frames_to_batch(ctx, size, image_dtype, mask_dtype, mc):
    """3 frames of 9 x 7, one flipped, each in another regime of the kernel"""
    from handobjectconsist_amd.datasets import frames as F

    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (3, 9, 7, 3), dtype=np.uint8)
    coeffs = np.array([[1.0, 0, 0, 0, 1.0, 0], [0.8, -0.3, 1.5, 0.3, 0.8, -1.0], [1.7, 0, -2.0, 0, 2.2, 1.0]])
    img, mask = F.frames_to_batch(ctx(frames), ctx.host(coeffs), size, flip=np.array([False, True, False]), mask_channels=mc,
                                  image_dtype=image_dtype, mask_dtype=mask_dtype)
    return dict(out=dict(image=img, jittermask=mask))


_frames_cases()


@case("color_augment-3x11x13")
def color_augment(ctx):
    """3 frames of 11 x 13, plans with blur"""
    from handobjectconsist_amd.datasets import frames as F
    from tests import coloraugm_ref as C

    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (3, 11, 13, 3), dtype=np.uint8)
    plans = np.zeros((3, 9), np.float32)
    plans[:, 0] = (0.5, 3.0, 0.0)
    plans[0, 1:5], plans[0, 5:9] = (C.OP_SATURATION, C.OP_CONTRAST, C.OP_HUE, C.OP_BRIGHTNESS), (1.4, 0.6, -30, 1.2)
    plans[2, 1], plans[2, 5] = C.OP_HUE, 38
    return dict(out=dict(frames=F.color_augment(ctx(frames), ctx.host(plans), flip=[0, 1, 0])))


@case("color_augment-1x3x5-contrast")
def color_augment_contrast(ctx):
    """one frame of 3 x 5 with a contrast op (the luma sum and the tail kernel) behind a blur: every region of the workspace --
    plans | luma sums | row-blurred frames -- is smaller than its 256-byte slot"""
    from handobjectconsist_amd.datasets import frames as F
    from tests import coloraugm_ref as C

    frames = np.random.default_rng(15).integers(0, 256, (1, 3, 5, 3), dtype=np.uint8)
    plans = np.zeros((1, 9), np.float32)
    plans[0, 0] = 1.5
    plans[0, 1:3], plans[0, 5:7] = (C.OP_BRIGHTNESS, C.OP_CONTRAST), (0.8, 1.3)
    return dict(out=dict(frames=F.color_augment(ctx(frames), ctx.host(plans), flip=[1])))


@case("jpeg_reconstruct-g17x9_s2", "g17x9_s2")
@case("jpeg_reconstruct-grey23x11", "grey23x11")
def jpeg_reconstruct(ctx, name):
    from handobjectconsist_amd.datasets import jpegdecode

    gold = np.load(os.path.join(GOLDEN, "jpeg_pil.npz"))
    packed = jpegdecode.entropy_decode(gold[name + "_stream"].tobytes())
    rgb = jpegdecode.reconstruct(ctx.host(packed[None]), ctx.dev)  # (host data: the upload is the entry point's own)
    assert np.array_equal(rgb[0].cpu().numpy(), gold[name + "_rgb"])
    return dict(out=dict(rgb=rgb))


@case("png_unfilter-37x29x3", False)
@case("png_unfilter-37x29x3-filter_per_frame", True)
def png_unfilter(ctx, batch):
    """(37 * 29 * 3) % 4 == 3: rows and frames start at bytes that are no multiple of 4"""
    from handobjectconsist_amd.datasets import pngdecode
    from tests import png_ref as R

    gold = np.load(os.path.join(GOLDEN, "png_pil.npz"))
    names = R.BATCH if batch else R.BATCH[:1]
    packed = np.stack([pngdecode.inflate(gold[n + "_stream"].tobytes()) for n in names])
    rgb = pngdecode.unfilter(ctx.host(packed), ctx.dev)  # (host data: the upload is the entry point's own)
    assert rgb.shape[1:] == (29, 37, 3) and np.array_equal(rgb.cpu().numpy(), np.stack([gold[n + "_rgb"] for n in names]))
    return dict(out=dict(rgb=rgb))


# --------------------------------------------------------------------------------------------------------------- the test
def _clear_caches():
    """module-level caches that hold device scratch or constants a run allocated (the pinned host words stay)"""
    from handobjectconsist_amd.neurender import rasterize
    from handobjectconsist_amd.warping import imgflowarp, opticalflow, pairstep

    for cache in (pairstep._PLANS, pairstep._FACES64, opticalflow._FACES2_CACHE, opticalflow._LUT_CACHE, opticalflow._LUT_BY_ID,
                  rasterize._BG_CACHE, imgflowarp._GRID_CACHE):
        cache.clear()


def _pinned_words():
    from handobjectconsist_amd.warping import opticalflow, pairstep

    return list(opticalflow._TILE_COUNTS.values()) + list(pairstep._COUNT_WORDS.values())


def _compare(name, got, want, tol):
    assert (got is None) == (want is None), f"{name}: present in one run only"
    if got is None:
        return
    assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride(), \
        f"{name}: {tuple(got.shape)} {got.dtype} {got.stride()} guarded, {tuple(want.shape)} {want.dtype} {want.stride()} plain"
    if tol is None:
        if not torch.equal(got, want):
            d = (got.double() - want.double()).abs()
            raise AssertionError(f"{name}: {int((~(d == 0)).sum())} of {d.numel()} elements differ from the plain run, max |diff| "
                                 f"{float(d[~torch.isnan(d)].max()) if bool((~torch.isnan(d)).any()) else float('nan'):g}, "
                                 f"{int(torch.isnan(got.double()).sum())} NaN guarded / {int(torch.isnan(want.double()).sum())} plain")
        return
    rtol, arel = tol
    g, w = got.double(), want.double()
    assert bool(torch.isfinite(g).all()), f"{name}: not finite"
    bound = arel * float(w.abs().max()) + rtol * w.abs()
    assert bool(((g - w).abs() <= bound).all()), f"{name}: max err {float((g - w).abs().max()):.3e} beyond the float-atomics tolerance"


STATS = {}


def _guarded_run(cuda, monkeypatch, name, leave_out=(), unguarded=None):
    """the guarded run of a case: (allocator, spied calls, the case's result, damaged bands, stranger pointers)"""
    from handobjectconsist_amd import _lib

    fn, args, kw = CASES[name]
    _clear_caches()
    alloc = G.GuardedAllocator(cuda, leave_out=leave_out)
    calls = []
    real_call, lib = _lib.call, _lib.load()
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append((n, a)), real_call(n, *a))[1])
    for entry in ("mr_pair_step_forward", "mr_pair_step_backward"):  # (pairstep calls them on the library: the block's pointers)
        def spy(block, stream, _real=getattr(lib, entry), _entry=entry):
            calls.append((_entry, (G.pair_step_pointers(block), stream)))
            return _real(block, stream)
        monkeypatch.setattr(lib, entry, spy)
    alloc.install(monkeypatch)
    try:
        guarded = fn(Ctx(cuda, alloc, monkeypatch, unguarded), *args, **kw)
        damage = alloc.check()
    finally:
        alloc.uninstall()
        monkeypatch.setattr(_lib, "call", real_call)
        _clear_caches()
    constants = list(guarded.get("const", ())) + _pinned_words()
    return alloc, calls, guarded, damage, alloc.pointer_report(calls, constants)


@pytest.mark.parametrize("name", list(CASES))
def test_guard_bands(cuda, monkeypatch, name):
    fn, args, kw = CASES[name]
    _clear_caches()
    plain = fn(Ctx(cuda, None, monkeypatch), *args, **kw)
    torch.cuda.synchronize()
    alloc, calls, guarded, damage, strangers = _guarded_run(cuda, monkeypatch, name)
    STATS[name] = dict(guarded_allocations=alloc.count(), rehomed=alloc.rehomed, calls=len(calls), pointer_arguments=alloc.pointers_seen)
    print(f"GUARD-BANDS {name}: {json.dumps(STATS[name])}")
    assert not damage, "\n".join(damage)                                                              # (a)
    assert not strangers, f"pointers outside every guarded interior and declared constant: {strangers[:8]} ({len(strangers)})"  # (b)
    assert calls and alloc.pointers_seen > 0, "the case reached no entry point"
    missing = set(guarded.get("wants_call", ())) - {n for n, _ in calls}
    assert not missing, f"the case did not reach {sorted(missing)}: {[n for n, _ in calls]}"
    assert set(guarded["out"]) == set(plain["out"])
    for key, got in guarded["out"].items():                                                           # (c)
        assert got is None or got.numel() == 0 or alloc.holds(got), f"{key}: not in guarded storage"
    for key, got in guarded["out"].items():                                                           # (d)
        _compare(key, None if got is None else got.detach(), None if plain["out"][key] is None else plain["out"][key].detach(),
                 guarded.get("loose", {}).get(key))


@pytest.mark.parametrize("name,leave_out,unguarded,entry,argument", [
    # _WarpFunction.forward allocates out / mask with torch.empty_like, its backward grad_x with torch.zeros_like
    ("warp-bilinear-1x1x3x2", ("empty_like",), None, "mr_warp_forward", 2),
    ("warp-bilinear-1x1x3x2", ("zeros_like",), None, "mr_warp_backward", 3),
    # get_occlusion_mask allocates its two outputs with torch.empty
    ("occlusion_mask-1x3x2", ("empty",), None, "mr_occlusion_mask", 7),
    # the first / the last test-made input of the case left out of guard(): x of warp, the gradient of its backward
    ("warp-bilinear-1x1x3x2", (), 0, "mr_warp_forward", 0),
    ("warp-bilinear-1x1x3x2", (), 2, "mr_warp_backward", 2),
])
def test_a_tensor_outside_the_guard_turns_the_pointer_check_red(cuda, monkeypatch, name, leave_out, unguarded, entry, argument):
    """Condition (b) is what makes the other three mean something: with one factory out of the patch list, or one input out of
    ``guard()``, the very argument that tensor is passed as is reported."""
    _alloc, _calls, _guarded, damage, strangers = _guarded_run(cuda, monkeypatch, name, leave_out, unguarded)
    assert not damage
    assert (entry, argument) in {(n, k) for n, k, _ in strangers}, strangers
