"""The Python layers on a side stream, behind a delay: every launch, memset and allocation of a call goes to the caller's
stream.  (tests/test_stream_record_host.py asks the same of the C entry points without a device; this file asks it of the
layers above them, on one.)

Mechanism.  The inputs of a call live in fixed buffers that first hold stale but valid content: NaN in floating-point tensors,
zero in every integer tensor a kernel uses as an index or a length, never garbage a kernel would turn into an address.  On a
side stream (bench.py's recipe: ``side.wait_stream(current)``, ``with torch.cuda.stream(side)``) the test issues a delay
kernel (``torch.cuda._sleep``, calibrated once per session with events to 20 ms -- the calls under test take well under 1 ms at
these shapes), then ``copy_`` of the real inputs into the buffers, then the layer under test with its backward.  A launch that
went to another stream runs ahead of the copy, on the stale content, and its results differ from those of the same call on the
default stream, made earlier in the test and synchronised.  ``test_the_mechanism_sees_a_stale_read`` shows with torch ops alone
that a default-stream read issued while the side stream sits behind the delay returns the stale content.

Rules.  Two default-stream calls are compared first; they have to give the same bits, and the side-stream call has to give
those bits: every forward output, mask, flow, coverage byte, the exact trunk cases.  The exceptions are listed output by
output (``ATOMIC``): sums the existing tests document as order-dependent because they meet in global fp32 atomics -- the pair
step's vertex gradients and warp's grad x (tests/test_gpu_raster.py's rule between two runs of the same products: "1e-5
relative + 1e-6 x max |ref|"), the head post-processing's grad scaletrans / grad st_obj over more than one block per sample
(tests/test_gpu_post_grads.py's rule against the float64 reference).  Where such an output has the default stream's bits
nothing more is asked; where not, its rule is.

Families here: ``rasterize_rgbad`` forward and backward ("scene" and "big" at B = 2, raster 64),
``opticalflow.flow_pair_loss`` through the struct path (case "A" of tests/pair_mesh_cases.py, two calls on the side stream,
the second with LIST_CLEAN, on a plan of its own), ``imgflowarp.warp`` / ``get_occlusion_mask`` /
``pair_consist`` (golden inputs, 7 x 5 and 64 x 64), ``bn_act``, the block tail and the stem pool with records backward on
tests/test_gpu_trunk_exact.py's / test_gpu_block_tail.py's exact inputs in fp32 and bf16 (also held to the exact
expectation), the MANO layer's network call and general call at B = 3, the head post-processing at (3, 1002).

... and ``RasterizeFunction`` (all five upstream-compatible entry points in one forward + backward, the hipMallocAsync /
hipFreeAsync pair of mr_backward_pixel_map among them), ``Renderer.render_vertex_colors``, the fused ``get_opticalflow`` at
B = 2 and raster 64, the stem's weight gradient through ``conv_stem_pool`` on exact inputs (fp32: the layer takes no other
image type), frames -> batch (fp32 and the compact batch), the colour augmentation, and the device stages of the JPEG and PNG
codecs on one golden stream each.

Measured on an MI355X (``SIDE-STREAM ...`` lines): 48 011 128 cycles of ``torch.cuda._sleep`` last 19.99 ms; the stale read is
seen.  Largest |side - default| per family: 0 for the pair step (losses, flows, coverage, all four vertex gradients, both
calls), the occlusion mask, pair_consist at all three sizes, bn_act, the block tail and the stem pool in both types, both MANO
calls; 2.4e-7 / 4.8e-7 for warp bilinear / nearest (grad x, fp32 atomics); 4.9e-4 / 2.4e-4 for rasterize_rgbad "scene" / "big"
(grad faces, fp32 atomics; everything else 0); 2.4e-4 on values of 1e3 for the head post-processing's grad
scaletrans / st_obj (fp32 atomics over four blocks per sample; 1.09e-7 against the float64 reference where the fp32
restatement has 4.23e-7); 0 for RasterizeFunction, render_vertex_colors, the fused get_opticalflow (their atomic gradients
had the default stream's bits too), conv_stem_pool, frames -> batch in both formats, the colour augmentation, JPEG and PNG.
Every ``ATOMIC`` output prints its case: whether the two default-stream calls agree, and whether the side stream has their bits.
"""
import os

import numpy as np
import pytest
import torch

from handobjectconsist_amd.utils import synth
from tests import geom_grad_cases as C
from tests import pair_mesh_cases as P
from tests import pair_oracle_harness as H

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DELAY_MS = 20.0
EXACT, ATOMIC = "same bits", "fp32 atomics"


@pytest.fixture(scope="session")
def delay(cuda):
    """cycles of torch.cuda._sleep that last DELAY_MS on this device, measured with events"""
    def ms_of(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms_of(100000)
    probe = 10_000_000
    cycles = int(probe * DELAY_MS / ms_of(probe))
    measured = ms_of(cycles)
    print(f"SIDE-STREAM delay: {cycles} cycles of torch.cuda._sleep last {measured:.2f} ms")
    assert 0.75 * DELAY_MS <= measured <= 3 * DELAY_MS, measured
    return cycles


def stale_like(t):
    return torch.full_like(t, float("nan")) if t.is_floating_point() else torch.zeros_like(t)


def on_side_stream(delay, real, fn):
    """``fn(*buffers)`` on a side stream behind the delay; the buffers get ``real``'s content on that stream, after the delay"""
    fixed = [stale_like(t) for t in real]
    torch.cuda.synchronize()
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        torch.cuda._sleep(delay)
        with torch.no_grad():
            for f, r in zip(fixed, real):
                f.copy_(r)
        out = fn(*fixed)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    return out


def on_default_stream(real, fn):
    out = fn(*[t.clone() for t in real])
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.detach().contiguous().view(torch.uint8)


def compare(family, names, kinds, side, first, second, rule=None):
    """the rules of this file's docstring; prints the family's largest difference.  ``rule(name, side tensor)``: the check the
    family's own test file documents for its order-dependent sums, in place of tests/test_gpu_raster.py's"""
    assert len(names) == len(kinds) == len(side) == len(first) == len(second), family
    worst, atomics = 0.0, []
    for name, kind, s, a, b in zip(names, kinds, side, first, second):
        if a is None:
            assert s is None and b is None, (family, name)
            continue
        assert s.shape == a.shape and s.dtype == a.dtype, (family, name)
        diff = float((s.double() - a.double()).abs().nan_to_num(0.0).max()) if s.numel() else 0.0
        worst = max(worst, diff)
        assert kind == ATOMIC or torch.equal(bits(a), bits(b)), f"{family}: {name} differs between two default-stream calls"
        if kind == ATOMIC:
            # which case this output is in on this run, output by output (agreement of two calls of an atomic sum proves no
            # fixed order: the head post-processing's two default-stream calls agreed where the third call did not)
            atomics.append(f"{name}: default calls {'agree' if torch.equal(bits(a), bits(b)) else 'differ'}, side "
                           f"{'has their bits' if torch.equal(bits(s), bits(a)) else f'differs by {diff:g} (under its rule)'}")
        if kind == EXACT:
            assert torch.equal(bits(s), bits(a)), f"{family}: {name} on the side stream differs from the default stream's (max |diff| {diff:g})"
        elif torch.equal(bits(s), bits(a)):
            pass
        elif rule is not None:
            rule(name, s)
        else:
            # (sums that meet in global fp32 atomics: two default-stream calls may agree by chance, the order is not fixed)
            ref = a.double()
            tol = 1e-5 * ref.abs() + 1e-6 * float(ref.abs().max())  # tests/test_gpu_raster.py: two runs of the same products
            assert bool(((s.double() - ref).abs() <= tol).all()), f"{family}: {name} beyond the rule of an order-dependent fp32 sum ({diff:g})"
    print(f"SIDE-STREAM {family}: largest |side - default| {worst:g} over {', '.join(names)}" + "".join("\n    " + a for a in atomics))


def run_family(delay, family, real, fn, names, kinds, rule=None):
    first, second = on_default_stream(real, fn), on_default_stream(real, fn)
    side = on_side_stream(delay, real, fn)
    compare(family, names, kinds, side, first, second, rule)
    return side


def up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- the mechanism ---------------------------------------------------------------------------------------------------------
def test_the_mechanism_sees_a_stale_read(cuda, delay):
    """torch ops only: while the side stream sits behind the delay, a clone issued on the default stream returns the stale
    content; after ``current.wait_stream(side)`` it returns the new one."""
    new = torch.arange(4096, dtype=torch.float32, device=cuda)
    fixed = stale_like(new)
    torch.cuda.synchronize()
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        torch.cuda._sleep(delay)
        fixed.copy_(new)
    early = fixed.clone()
    cur.wait_stream(side)
    late = fixed.clone()
    torch.cuda.synchronize()
    assert bool(torch.isnan(early).all()), ("the device serialised the two streams: a default-stream read issued behind the side stream's "
                                            "delay saw the new content, so this file's tests could not see a launch on the wrong stream")
    assert torch.equal(late, new)


# ---- the pair step -------------------------------------------------------------------------------------------------------------
def test_pair_step_struct_path(cuda, delay, monkeypatch):
    from handobjectconsist_amd.neurender.renderer import Renderer
    from handobjectconsist_amd.warping import opticalflow, pairstep

    H.clear_caches()
    monkeypatch.setattr(opticalflow, "DEBUG_POISON_RENDER_OUTPUTS", False)
    monkeypatch.setattr(opticalflow, "USE_PAIR_STEP", True)
    name = "A"
    case = H.CASES[name]
    B, is_ = case["B"], case["raster"]
    s = H.oracle_forward(name, case["seed"])["scene"]
    Rm, tm, dm = P.camera(B, case["per_sample_cam"])
    ren = Renderer(image_size=is_, R=up(Rm, cuda), t=up(tm, cuda), K=up(np.ones((1, 3, 3), np.float32), cuda), dist_coeffs=up(dm, cuda),
                   orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True, light_intensity_ambient=0.8)
    keys = ("hand_verts1", "obj_verts1", "hand_verts2", "obj_verts2", "K1", "K2", "hand_faces", "obj_faces")
    real = [up(np.asarray(s[k], np.int64) if "faces" in k else s[k], cuda) for k in keys] + [up(x, cuda) for x in H.images(case, case["seed"], False)]
    w = [up(x, cuda) for x in H.weights(B)]
    Wd, Hh = H.crop(case)

    def one(h1, o1, h2, o2, K1, K2, hf, of, im_ref, im, jm_ref, jm):
        leaves = [x.detach().requires_grad_(True) for x in (h1, o1, h2, o2)]
        res = opticalflow.flow_pair_loss([(leaves[0], leaves[1]), (leaves[2], leaves[3])], (hf, of), [K1, K2], ren, H.crop(case), im_ref, im,
                                         jm_ref, jm, ignore_face_idxs=synth.HAND_IGNORE_FACES, with_sum=True, with_mean="sum",
                                         criterion=H.crit_code("l1"))
        assert res is not None
        lf, lb, flows, lsum, mean = res
        grads = torch.autograd.grad((lf * w[0]).sum() + (lb * w[1]).sum() + (lsum * w[2]).sum() + H.WM * mean, leaves)
        base = flows[0]._base
        hit = base._hoc_coverage[0]
        # the flows are defined under covered tiles only: zero elsewhere, by the coverage words, before they are compared
        words = hit.contiguous().view(torch.int32).view(2 * B, (is_ + 7) // 8, (is_ + 31) // 32) != 0
        yy, xx = torch.meshgrid(torch.arange(Hh, device=cuda), torch.arange(Wd, device=cuda), indexing="ij")
        defined = words[:, (is_ - 1 - yy) >> 3, xx >> 5]
        shown = torch.where(defined[..., None], base.detach(), torch.zeros_like(base))
        return [lf.detach(), lb.detach(), lsum.detach(), mean.detach().reshape(1), shown, hit.clone()] + list(grads)

    def fn(*args):
        # two calls: the second runs on the list header the first left clean
        first = one(*args)
        plan = [p for k, p in pairstep._PLANS.items() if k[1] == torch.cuda.current_stream().cuda_stream]
        assert len(plan) == 1 and plan[0].list_clean
        out = first + one(*args)
        assert plan[0].st.flags & pairstep.LIST_CLEAN
        return out

    one_names = ["loss_fwd", "loss_bwd", "loss sum", "mean", "flows", "coverage bytes"] + [f"d/d {leaf}" for leaf in H.LEAVES]
    one_kinds = [EXACT] * 6 + [ATOMIC] * 4
    try:
        run_family(delay, "flow_pair_loss, struct path", real, fn, one_names + [n + " (second call)" for n in one_names], one_kinds * 2)
        assert len(pairstep._PLANS) == 2, "the side stream's calls go through a plan of their own"
        (k0, p0), (k1, p1) = pairstep._PLANS.items()
        assert p0 is not p1 and k0[1] != k1[1] and k0[:1] + k0[2:] == k1[:1] + k1[2:]
    finally:
        H.clear_caches()


# ---- the generic render ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scene", "big"])
def test_rasterize_rgbad(cuda, delay, kind):
    from handobjectconsist_amd.neurender import rasterize
    from tests import test_gpu_raster as TR

    B, is_ = 2, 64
    faces, tex = TR.make_case(kind, B, is_, 5)
    rng = np.random.default_rng(105)
    grads = [rng.standard_normal(s).astype(np.float32) for s in ((B, 3, is_, is_), (B, is_, is_), (B, is_, is_))]
    real = [TR.t(faces, cuda), TR.t(tex, cuda)] + [up(g, cuda) for g in grads]

    def fn(f, x, g_rgb, g_alpha, g_depth):
        f, x = f.requires_grad_(True), x.requires_grad_(True)
        out = rasterize.rasterize_rgbad(f, x, is_, False, 0.1, 100, 1e-3, (0.0, 0.0, 0.0))
        gf, gx = torch.autograd.grad([out["rgb"], out["alpha"], out["depth"]], [f, x], [g_rgb, g_alpha, g_depth])
        return [out["rgb"].detach(), out["alpha"].detach(), out["depth"].detach(), gf, gx]

    # (grad faces: kernel D by strips, whose sums meet in float atomics; grad textures: the gather, deterministic --
    # tests/test_gpu_raster.py asserts both)
    side = run_family(delay, f"rasterize_rgbad {kind} B=2 raster 64", real, fn, ["rgb", "alpha", "depth", "grad faces", "grad textures"],
                      [EXACT, EXACT, EXACT, ATOMIC, EXACT])
    assert float(side[3].abs().max()) > 0 and float(side[4].abs().max()) > 0


# ---- warp, occlusion, pair loss ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_warp(cuda, delay, mode):
    from handobjectconsist_amd.warping import imgflowarp

    g = np.load(os.path.join(GOLDEN, "warp_basic.npz"))
    real = [up(g[k], cuda) for k in ("x", "flow", "grad_out")]

    def fn(x, flow, grad_out):
        x, flow = x.requires_grad_(True), flow.requires_grad_(True)
        out, mask = imgflowarp.warp(x, flow, mode=mode)
        gx, gf = torch.autograd.grad((out * grad_out).sum(), [x, flow], allow_unused=True)
        return [out.detach(), mask, gx, gf]

    run_family(delay, f"imgflowarp.warp {mode}", real, fn, ["out", "mask", "grad x", "grad flow"], [EXACT, EXACT, ATOMIC, EXACT])


def test_occlusion_mask(cuda, delay):
    from handobjectconsist_amd.warping import imgflowarp

    g = np.load(os.path.join(GOLDEN, "warp_occlusion.npz"))
    real = [up(g[k], cuda) for k in ("mask_flow1", "mask_flow2", "flow12", "flow21")]
    side = run_family(delay, "get_occlusion_mask", real, lambda *a: list(imgflowarp.get_occlusion_mask(*a)), ["occl1", "occl2"], [EXACT] * 2)
    assert float(side[0].sum()) > 10


def _pair_consist_inputs(cuda, shape):
    if shape is None:
        g = np.load(os.path.join(GOLDEN, "warp_pair_consist.npz"))
        return [up(g[k], cuda) for k in ("flow12", "flow21", "image_ref", "image", "jitter_ref", "jitter", "grad_loss")]
    B, Hh, Wd = shape
    rng = np.random.default_rng(75)
    f32 = lambda a: up(a.astype(np.float32), cuda)
    flows = [f32(rng.uniform(-2, 2, (B, Hh, Wd, 2))) for _ in range(2)]
    images = [f32(rng.uniform(0, 1, (B, 3, Hh, Wd))) for _ in range(2)]
    jitter = [f32(rng.uniform(0, 1, (B, 3, Hh, Wd)) > 0.2) for _ in range(2)]
    return flows + images + jitter + [f32(rng.uniform(0.5, 1.5, (B,)))]


@pytest.mark.parametrize("shape", [None, (2, 7, 5), (2, 64, 64)], ids=["golden", "7x5", "64x64"])
def test_pair_consist(cuda, delay, shape):
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    real = _pair_consist_inputs(cuda, shape)

    def fn(f12, f21, im_ref, im, jm_ref, jm, gl):
        f12, f21 = f12.requires_grad_(True), f21.requires_grad_(True)
        loss, masks, warps, diffs = imgflowarp.pair_consist([f12, f21], im_ref, im, jm_ref, jm, PyramidCriterion("l1"), use_backward=True, outputs="full")
        g12, g21 = torch.autograd.grad((loss * gl).sum(), [f12, f21])
        return [loss.detach(), g12, g21, masks[0]["full_mask"], masks[1]["full_mask"], warps[0], warps[1]]

    run_family(delay, f"pair_consist {shape or 'golden'}", real, fn, ["loss", "grad flow12", "grad flow21", "full mask 1", "full mask 2", "warp 1", "warp 2"],
               [EXACT] * 7)


# ---- trunk glue on the exact inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("op,shape,cl,with_res", [("bn", (3, 8, 4, 4), False, True), ("bn", (2, 8, 3, 5), True, False), ("stem", (2, 4, 35, 70), True, False)],
                         ids=["bn_act-nchw-residual", "bn_act-nhwc", "stem_pool-records"])
def test_trunk_glue_exact(cuda, delay, op, shape, cl, with_res, dtype):
    from handobjectconsist_amd.nn import frozen_bn
    from tests import test_gpu_trunk_exact as TX

    c = TX._case(op, shape, True, with_res)
    bn = TX._module(cuda, shape[1], c.weight, c.bias, c.mean)
    real = [TX._put(c.x, cuda, dtype, cl)] + ([TX._put(c.r, cuda, dtype, cl)] if with_res else [])
    y_cl = cl  # (the outputs of channels-last inputs are channels-last)
    real += [TX._put(c.gy, cuda, dtype, y_cl), TX._put(c.gy2, cuda, dtype, y_cl)]

    def fn(x, *rest):
        r = rest[0].requires_grad_(True) if with_res else None
        gy, gy2 = rest[-2:]
        x = x.requires_grad_(True)
        y1, y2 = frozen_bn.bn_act(x, bn, residual=r, relu=True, dup=True) if op == "bn" else frozen_bn.stem_pool(x, bn, dup=True)
        assert y1.stride() == gy.stride()
        grads = torch.autograd.grad([y1, y2], [x, bn.weight, bn.bias] + ([r] if with_res else []), [gy, gy2])
        return [y1.detach()] + list(grads) + ([] if with_res else [None])

    names = ["y", "grad x", "grad weight", "grad bias", "grad residual"]
    side = run_family(delay, f"{op} {shape} {'nhwc' if cl else 'nchw'} {str(dtype)[6:]}", real, fn, names, [EXACT] * 5)
    ref = TX._ref64(op, shape, True, with_res, "both")
    for name, got, want, cast in zip(names, side, (ref.y, ref.gx, ref.gw, ref.gb, ref.gr), (dtype, dtype, torch.float32, torch.float32, dtype)):
        if got is not None:
            TX._same(got.contiguous(), want.to(cuda).to(cast), f"{op} {shape} on the side stream: {name} against the exact expectation")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_block_tail_exact(cuda, delay, dtype):
    from handobjectconsist_amd.nn import frozen_bn
    from tests import test_gpu_block_tail as TB

    shape = TB.SMALL[0]
    c = TB._case(shape)
    bn = TB._module(cuda, shape[1], c.weight, c.bias, c.mean, True, True)
    bn_d = TB._module(cuda, shape[1], c.weight_d, c.bias_d, c.mean_d, True, True)
    real = [TB._put(t, cuda, dtype) for t in (c.x, c.xd, c.gy, c.gy2)]

    def fn(x, xd, gy, gy2):
        x, xd = x.requires_grad_(True), xd.requires_grad_(True)
        y1, y2 = frozen_bn.bn_add_bn_act(x, bn, xd, bn_d, dup=True)
        return [y1.detach()] + list(torch.autograd.grad([y1, y2], [x, xd, bn.weight, bn.bias, bn_d.weight, bn_d.bias], [gy, gy2]))

    names = ["y", "gx", "gxd", "gw", "gb", "gwd", "gbd"]
    side = run_family(delay, f"block tail {shape} {str(dtype)[6:]}", real, fn, names, [EXACT] * 7)
    ref = TB._ref64(shape, "both")
    for name, got in zip(names, side):
        cast = dtype if name in ("y", "gx", "gxd") else torch.float32
        TB._same(got.contiguous(), getattr(ref, name).to(cuda).to(cast).contiguous(), f"block tail on the side stream: {name} against the exact expectation")


# ---- MANO and the head post-processing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["forward-pca-centre9", "full-pca-centre9-trans"], ids=["network-call", "general-call"])
def test_mano_layer(cuda, delay, variant):
    layer = C.make_layer(variant).to(cuda)
    entry = C.MANO_VARIANTS[variant][0]
    pose, betas, trans, wv, wj = (None if a is None else a[:3].to(cuda) for a in C.mano_inputs(variant) + C.mano_weights("dense"))
    real = [pose, betas] + ([trans] if trans is not None else [])
    names = ["verts", "joints", "pose", "betas"] + (["trans"] if trans is not None else [])

    def fn(p, b, t=None):
        out = C.mano_run(layer, entry, p, b, t, wv, wj)
        return [out[k] for k in names]

    run_family(delay, f"MANO layer {variant} B=3", real, fn, names, [EXACT] * len(names))


def test_meshreg_post(cuda, delay):
    from handobjectconsist_amd import _lib

    shape = (3, 778, 21, 1002)
    tf, sf, off_z, (rw, rh) = C.POST_CONSTS
    real = [up(a, cuda) for a in C.post_inputs(shape)] + [up(a, cuda) for a in C.post_weights(shape)]
    out_shapes = [(3, 778, 3), (3, 21, 3), (3, 21, 2), (3, 1002, 3), (3, 1002, 2)]

    def fn(*t):
        ins, gin = t[:6], t[6:]
        outs = [torch.empty(s, dtype=torch.float32, device=cuda) for s in out_shapes]
        _lib.call("mr_meshreg_post_forward", *[_lib.ptr(x) for x in ins], tf, sf, off_z, rw, rh, *[_lib.ptr(o) for o in outs], *shape,
                  _lib.stream_ptr(cuda))
        work = torch.empty((shape[0] * 15,), dtype=torch.float32, device=cuda)
        grads = [torch.empty_like(x) for x in ins[:4]]
        _lib.call("mr_meshreg_post_backward", *[_lib.ptr(x) for x in ins], tf, sf, off_z, rw, rh, *[_lib.ptr(g) for g in gin], _lib.ptr(work),
                  *[_lib.ptr(g) for g in grads], *shape, _lib.stream_ptr(cuda))
        return outs + grads

    # grad scaletrans / st_obj: per-sample sums of several blocks' float atomics (tests/test_gpu_post_grads.py: only "a sample
    # whose points fit one block ... nothing to reorder" gives the same bits twice).  That file's rule for them: four times the
    # error of the fp32 restatement against the float64 reference, per sample
    subset = (0, 1, 2, 3, 4)

    def rule(name, got):
        k = ["grad " + n for n in C.POST_GRADS].index(name)
        ref, yard = C.post_reference(shape, subset)[1][k], C.post_reference(shape, subset, torch.float32)[1][k]
        report = C.Report(f"SIDE-STREAM post {shape} {name}")
        report.add(name, got.cpu().numpy(), yard, ref, C.MAX_EY_GRAD)
        report.finish()

    run_family(delay, "meshreg_post (3, 1002)", real, fn, list(C.POST_OUTPUTS) + ["grad " + n for n in C.POST_GRADS], [EXACT] * 7 + [ATOMIC] * 2, rule)


# ---- the upstream-compatible autograd op, the vertex-colour render, the fused flows ------------------------------------------------
def test_rasterize_function_five_entry_points(cuda, delay):
    """RasterizeFunction with rgb, alpha and depth: mr_forward_face_index_map, mr_forward_texture_sampling and, in the
    backward, mr_backward_pixel_map (whose workspace is a hipMallocAsync / hipFreeAsync pair on the caller's stream),
    mr_backward_textures and mr_backward_depth_map"""
    from handobjectconsist_amd.neurender import rasterize
    from tests import test_gpu_raster as TR

    B, is_ = 2, 64
    faces, tex = TR.make_case("scene", B, is_, 6)
    rng = np.random.default_rng(106)
    grads = [rng.standard_normal(s).astype(np.float32) for s in ((B, is_, is_, 3), (B, is_, is_), (B, is_, is_))]
    real = [TR.t(faces, cuda), TR.t(tex, cuda)] + [up(g, cuda) for g in grads]

    def fn(f, x, g_rgb, g_alpha, g_depth):
        f, x = f.requires_grad_(True), x.requires_grad_(True)
        rgb, alpha, depth, fim, inv, wmap = rasterize.RasterizeFunction.apply(f, x, is_, 0.1, 100, 1e-3, (0.0, 0.0, 0.0), True, True, True)
        gf, gx = torch.autograd.grad([rgb, alpha, depth], [f, x], [g_rgb, g_alpha, g_depth])
        return [rgb.detach(), alpha.detach(), depth.detach(), fim, inv.detach(), wmap.detach(), gf, gx]

    # (both gradients accumulate with float atomics: include/meshraster_hip.h on mr_backward_textures / _depth_map, and kernel
    # D's strips)
    side = run_family(delay, "RasterizeFunction B=2 raster 64", real, fn,
                      ["rgb map", "alpha map", "depth map", "face index map", "face inverse map", "weight map", "grad faces", "grad textures"],
                      [EXACT] * 6 + [ATOMIC] * 2)
    assert int((side[3] >= 0).sum()) > 100 and float(side[6].abs().max()) > 0 and float(side[7].abs().max()) > 0


def _scene(cuda, seed):
    from handobjectconsist_amd.neurender.renderer import Renderer

    B, is_ = 2, 64
    s = synth.random_scene(B, seed=seed, image_size=is_)
    ren = Renderer(image_size=is_, R=torch.eye(3, device=cuda)[None], t=torch.zeros(1, 3, device=cuda), K=torch.ones(1, 3, 3, device=cuda),
                   orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True)
    return B, is_, s, ren


def test_render_vertex_colors(cuda, delay):
    B, is_, s, ren = _scene(cuda, 12)
    g = torch.Generator().manual_seed(2)
    real = [up(s["verts1"], cuda), up(s["faces"], cuda), torch.randn(B, s["verts1"].shape[1], 3, generator=g).to(cuda), up(s["K1"], cuda),
            torch.randn(B, 3, is_, is_, generator=g).to(cuda)]

    def fn(verts, faces, cols, K1, g_rgb):
        cols = cols.requires_grad_(True)
        out = ren.render_vertex_colors(verts, faces, cols, K=K1)
        (gc,) = torch.autograd.grad((out["rgb"] * g_rgb).sum(), cols)
        return [out["rgb"].detach(), out["face_index_map"], gc]

    side = run_family(delay, "Renderer.render_vertex_colors B=2 raster 64", real, fn, ["rgb", "face index map", "grad colours"], [EXACT, EXACT, ATOMIC])
    assert int((side[1] >= 0).sum()) > 100 and float(side[2].abs().max()) > 0


def test_get_opticalflow_fused(cuda, delay):
    from handobjectconsist_amd.warping import opticalflow

    B, is_, s, ren = _scene(cuda, 3)
    H.clear_caches()
    real = [up(s[k], cuda) for k in ("verts1", "verts2", "faces", "K1", "K2")]
    real.append(torch.randn(B, is_, is_, 2, generator=torch.Generator().manual_seed(5)).to(cuda))

    def fn(v1, v2, faces, K1, K2, gf):
        v1, v2 = v1.requires_grad_(True), v2.requires_grad_(True)
        flows = opticalflow.get_opticalflow([v1, v2], faces, [K1, K2], ren, orig_img_size=(is_, is_), ignore_face_idxs=synth.HAND_IGNORE_FACES)
        g1, g2 = torch.autograd.grad((flows[0] * gf).sum() + (flows[1] * gf).sum(), [v1, v2])
        return [flows[0].detach(), flows[1].detach(), g1, g2]

    try:
        side = run_family(delay, "get_opticalflow, fused, B=2 raster 64", real, fn, ["flow12", "flow21", "grad verts1", "grad verts2"],
                          [EXACT, EXACT, ATOMIC, ATOMIC])
        assert float(side[0].abs().max()) > 0 and float(side[2].abs().max()) > 0
    finally:
        H.clear_caches()


# ---- the stem's weight gradient through the Python layer ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 23, 19)], ids=str)
def test_stem_weight_gradient_exact(cuda, delay, shape):
    """conv_stem_pool (fp32 only: conv_stem_applies) on tests/test_gpu_stem_wrw.py's exact inputs with a small-integer
    convolution weight: the pooled output, the convolution's weight gradient (mr_stem_conv_wrw) and the BatchNorm's
    (mr_stem_pool_param_grads), against the default stream and against explicit fp64 torch ops on the CPU"""
    import torch.nn.functional as F

    from handobjectconsist_amd.nn import frozen_bn
    from tests import test_gpu_stem_wrw as TW

    image, _, g1, g2, w, b, m = TW._inputs(shape, True)
    cw = torch.randint(-2, 3, (TW.C, 3, 7, 7), generator=torch.Generator().manual_seed(31)).float()
    conv = torch.nn.Conv2d(3, TW.C, 7, 2, 3, bias=False).to(cuda).to(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(TW.C, eps=TW.EPS).to(cuda).eval()
    with torch.no_grad():
        conv.weight.copy_(cw)
        bn.weight.copy_(w)
        bn.bias.copy_(b)
        bn.running_mean.copy_(m)
        bn.running_var.fill_(TW.VAR)
    cl = lambda t: t.to(cuda).contiguous(memory_format=torch.channels_last)
    real = [cl(image), cl(g1), cl(g2)]

    def fn(img, gy, gy2):
        y1, y2 = frozen_bn.conv_stem_pool(img, conv, bn, dup=True)
        return [y1.detach()] + list(torch.autograd.grad([y1, y2], [conv.weight, bn.weight, bn.bias], [gy, gy2]))

    names = ["y", "grad conv weight", "grad bn weight", "grad bn bias"]
    side = run_family(delay, f"conv_stem_pool {shape}", real, fn, names, [EXACT] * 4)
    d = torch.float64
    cw64, w64, b64 = (t.to(d).requires_grad_(True) for t in (cw, w, b))
    z = (F.conv2d(image.to(d), cw64, None, 2, 3) - m.to(d)[None, :, None, None]) * (w64 / torch.sqrt(torch.full((TW.C,), TW.VAR, dtype=d) + TW.EPS))[None, :, None, None] \
        + b64[None, :, None, None]
    y = F.max_pool2d(F.relu(z), 3, 2, 1)
    y.backward((g1 + g2).to(d))
    for name, got, want in zip(names, side, (y.detach(), cw64.grad, w64.grad, b64.grad)):
        assert float(want.abs().max()) < 2 ** 24
        TW._same(got.contiguous().cpu(), want.float().contiguous(), f"conv_stem_pool {shape} on the side stream: {name} against the exact expectation")


# ---- the dataset pipeline: frames -> batch, colour augmentation, JPEG, PNG -------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True], ids=["fp32", "bf16-u8"])
def test_frames_to_batch(cuda, delay, compact):
    from handobjectconsist_amd.datasets import frames as F

    gold = np.load(os.path.join(GOLDEN, "augment_pil.npz"))
    case = 0
    W, Hh = (int(v) for v in gold[f"c{case}_size"])
    coeffs = np.asarray(gold[f"c{case}_coeffs"][None], np.float64)
    kw = dict(image_dtype=torch.bfloat16, mask_dtype=torch.uint8) if compact else {}
    side = run_family(delay, f"frames_to_batch golden case {case} {'compact' if compact else 'fp32'}", [up(gold[f"c{case}_src"][None], cuda)],
                      lambda frames: list(F.frames_to_batch(frames, coeffs, (W, Hh), **kw)), ["image", "jitter mask"], [EXACT] * 2)
    if not compact:
        assert np.array_equal(side[0][0].cpu().numpy(), gold[f"c{case}_image"]) and np.array_equal(side[1][0].cpu().numpy(), gold[f"c{case}_jittermask"])


def test_color_augment(cuda, delay):
    from handobjectconsist_amd.datasets import frames as F

    import json

    gold = np.load(os.path.join(GOLDEN, "coloraugm_pil.npz"))
    # (the first golden case of more than a few pixels that blurs and has ops)
    case = next(c for c in range(json.loads(str(gold["meta"]))["cases"])
                if gold[f"c{c}_in"].size >= 1500 and gold[f"c{c}_plan"][0, 0] > 0 and gold[f"c{c}_plan"][0, 1] != 0)
    plans, flip = gold[f"c{case}_plan"], gold[f"c{case}_flip"]
    side = run_family(delay, f"color_augment golden case {case}", [up(gold[f"c{case}_in"], cuda)], lambda frames: [F.color_augment(frames, plans, flip=flip)],
                      ["frames"], [EXACT])
    assert np.array_equal(side[0].cpu().numpy(), gold[f"c{case}_out"])


@pytest.mark.parametrize("codec", ["jpeg", "png"])
def test_packed_frame_codecs(cuda, delay, codec):
    """the device stage of one golden stream: the packed frame (a byte stream: zeros while stale) in the fixed buffer, the
    geometry from the host as the Python layer passes it"""
    import json

    from handobjectconsist_amd.datasets import jpegdecode, pngdecode

    gold = np.load(os.path.join(GOLDEN, f"{codec}_pil.npz"))
    name = next(n for n in json.loads(str(gold["meta"]))["names"] if gold[n + "_rgb"].shape[0] * gold[n + "_rgb"].shape[1] >= 1000)
    mod = jpegdecode if codec == "jpeg" else pngdecode
    packed = (mod.entropy_decode if codec == "jpeg" else mod.inflate)(gold[name + "_stream"].tobytes())[None]
    geom = mod.batch_geometry(packed)
    want = gold[name + "_rgb"]

    def fn(packed_d):
        out = torch.empty((1,) + want.shape, dtype=torch.uint8, device=cuda)
        mod._device_stage(packed_d, 1, geom, out, cuda)
        return [out]

    side = run_family(delay, f"{codec} device stage, golden stream {name}", [up(np.ascontiguousarray(packed), cuda)], fn, ["frames"], [EXACT])
    assert np.array_equal(side[0][0].cpu().numpy(), want)
