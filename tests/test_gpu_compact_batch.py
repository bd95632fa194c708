"""The compact image batch (bf16 images, uint8 jitter masks) on the GPU: the frame kernel's typed outputs
against its fp32 outputs (round-to-nearest-even, mask == 1), and the fused pair kernels on a compact batch against the same
kernels on the widened batch -- widening bf16 / u8 to fp32 is exact, so everything but the atomically accumulated vertex
gradients is compared bit for bit -- plus the derived distance of the compact path from the fp32 one on the metric scene."""
import json
import os

import numpy as np
import pytest
import torch

from handobjectconsist_amd.utils import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = np.load(os.path.join(GOLDEN, "augment_pil.npz"))
BF16, U8, F32 = torch.bfloat16, torch.uint8, torch.float32


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e}, {(err > tol).sum()} / {err.size} out of tol"


# ---------------------------------------------------------------------------------------------------
# frames -> batch
# ---------------------------------------------------------------------------------------------------


def _check_frames(cuda, frames, coeffs, size, what, flip=None, mask_channels=3, **kw):
    """every pair of output types against the fp32 batch of the same call: image_bf16 == image_fp32.bfloat16() (torch's cast
    rounds to nearest-even), mask_u8 == (mask_fp32 == 1); returns the fp32 batch"""
    from handobjectconsist_amd.datasets import frames as F

    fr = frames if torch.is_tensor(frames) else t(frames, cuda)
    co = np.asarray(coeffs, np.float64)
    img, mask = F.frames_to_batch(fr, co, size, flip=flip, mask_channels=mask_channels, **kw)
    assert img.dtype == F32 and mask.dtype == F32
    for idt, mdt in ((BF16, U8), (BF16, F32), (F32, U8)):
        img_c, mask_c = F.frames_to_batch(fr, co, size, flip=flip, mask_channels=mask_channels, image_dtype=idt, mask_dtype=mdt, **kw)
        assert img_c.dtype == idt and mask_c.dtype == mdt and img_c.shape == img.shape and mask_c.shape == mask.shape
        assert torch.equal(img_c, img.to(idt)), (what, "image", idt)
        assert torch.equal(mask_c, (mask == 1).to(mdt)), (what, "mask", mdt)
    return img, mask


@pytest.mark.parametrize("case", range(len(GOLD["kinds"])))
def test_frame_kernel_golden_cases(cuda, case):
    W, H = (int(v) for v in GOLD[f"c{case}_size"])
    img, mask = _check_frames(cuda, GOLD[f"c{case}_src"][None], GOLD[f"c{case}_coeffs"][None], (W, H), GOLD["kinds"][case])
    assert np.array_equal(img[0].cpu().numpy(), GOLD[f"c{case}_image"])  # (the fp32 batch is still the fixture's)
    assert np.array_equal(mask[0].cpu().numpy(), GOLD[f"c{case}_jittermask"])


def test_frame_kernel_at_the_shape_of_a_step(cuda):
    """192 frames of 640 x 480 -> 256 x 256 (3 x 64 frames of a step) with the dataset's own crop affines, rotations and flips;
    normalisation constants other than (0.5, 1); one and three mask channels."""
    from handobjectconsist_amd.datasets import handutils

    rng = np.random.default_rng(3)
    N, Hs, Ws, res = 192, 480, 640, (256, 256)
    frames = t(rng.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8), cuda)
    affs = np.stack([handutils.pil_coeffs(handutils.get_affine_transform(rng.uniform((200, 150), (440, 330)), rng.uniform(150, 500), res,
                                                                         rot=(0, 0.3, 0, -0.2)[k % 4])[0]) for k in range(N)])
    flip = rng.random(N) < 0.5
    img, mask = _check_frames(cuda, frames, affs, res, "step shape", flip=flip)
    assert 0.2 < float(mask.mean()) < 1.0 and float(img.float().abs().max()) <= 0.5
    _check_frames(cuda, frames[:16], affs[:16], res, "normalised", flip=flip[:16], mask_channels=1,
                  mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def test_frame_kernel_mixed_regimes_flips_and_odd_widths(cuda):
    """Per-frame regimes (scale / fixed point / double) and flips in one batch; widths that are not multiples of the 4-pixel
    store take the scalar tail, whose elements are 2 and 1 bytes here; 1-pixel outputs."""
    from tests.test_gpu_frames import _random_coeffs

    rng = np.random.default_rng(12)
    odd = 0
    for trial in range(30):
        N, Hs, Ws = int(rng.integers(1, 7)), int(rng.integers(1, 70)), int(rng.integers(1, 70))
        W, H = int(rng.integers(1, 80)), int(rng.integers(1, 60))
        if trial < 4:
            W = (1, 2, 3, 5)[trial]
        odd += W % 4 != 0
        frames = rng.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8)
        coeffs = [_random_coeffs(rng, int(rng.integers(0, 4)), Ws, Hs, W, H) for _ in range(N)]
        _check_frames(cuda, frames, coeffs, (W, H), ("mixed", trial), flip=rng.random(N) < 0.4, mask_channels=1 if trial % 3 == 0 else 3)
    assert odd >= 10


def test_frame_kernel_edge_cases(cuda):
    from handobjectconsist_amd.datasets import frames as F

    frames = torch.zeros((2, 5, 6, 3), dtype=torch.uint8, device=cuda)
    ident = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (2, 1))
    img, mask = F.frames_to_batch(frames[:0], ident[:0], (4, 4), image_dtype=BF16, mask_dtype=U8)  # empty batch
    assert img.shape == (0, 3, 4, 4) and mask.shape == (0, 3, 4, 4) and img.dtype == BF16 and mask.dtype == U8
    bad = ident.copy()
    bad[1, 2] = np.nan  # non-finite coefficients: an empty frame
    bad2 = ident.copy()
    bad2[0, 4] = np.inf
    for co in (bad, bad2):
        _check_frames(cuda, frames + 9, co, (4, 4), "non-finite")
    img, mask = F.frames_to_batch(frames + 9, bad, (4, 4), image_dtype=BF16, mask_dtype=U8)
    assert bool((mask[1] == 0).all()) and bool((img[1] == -0.5).all()) and bool((mask[0] == 1).all())
    img, mask = F.frames_to_batch(frames, ident, (4, 4), jittermask=False, image_dtype=BF16, mask_dtype=U8)
    assert mask is None and img.dtype == BF16
    with pytest.raises(RuntimeError):
        F.frames_to_batch(frames, ident, (4, 4), mask_channels=2, image_dtype=BF16, mask_dtype=U8)
    # a zero std: inf / NaN table entries round like torch's cast (NaN -> the quiet NaN)
    img32, _ = F.frames_to_batch(frames + 128, ident, (4, 4), mean=(0.5, 0.5, 128 / 255), std=(1.0, 0.0, 0.0))
    img16, _ = F.frames_to_batch(frames + 128, ident, (4, 4), mean=(0.5, 0.5, 128 / 255), std=(1.0, 0.0, 0.0), image_dtype=BF16)
    assert torch.isinf(img32[:, 1]).all() and torch.equal(img16.view(torch.int16), img32.bfloat16().view(torch.int16))


def test_fp32_entry_point_and_typed_f32_entry_point_are_bit_identical(cuda):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import frames as F

    rng = np.random.default_rng(8)
    for N, Hs, Ws, W, H in ((6, 120, 160, 64, 64), (3, 33, 47, 31, 18)):
        frames = t(rng.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8), cuda)
        th = rng.uniform(-0.4, 0.4, N)
        coeffs = np.stack([[1.7 * np.cos(a), -1.7 * np.sin(a), 3.0, 1.7 * np.sin(a), 1.7 * np.cos(a), -2.0] for a in th])
        coeffs[0] = [1.5, 0, 2.25, 0, 1.5, -1.0]
        img, mask = F.frames_to_batch(frames, coeffs, (W, H))
        co = t(coeffs, cuda)
        img2, mask2 = torch.full_like(img, float("nan")), torch.full_like(mask, float("nan"))
        wbytes = int(_lib.load().mr_frames_to_batch_workspace_bytes(N, H, W))
        work = torch.empty((wbytes,), dtype=torch.uint8, device=cuda)
        _lib.call("mr_frames_to_batch_typed", _lib.ptr(frames), _lib.ptr(co), None, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0, _lib.ptr(work), wbytes,
                  _lib.ptr(img2), _lib.ptr(mask2), 3, N, Hs, Ws, H, W, _lib.stream_ptr(cuda), _lib.DTYPE_F32, _lib.DTYPE_F32)
        assert torch.equal(img2.view(torch.int32), img.view(torch.int32)) and torch.equal(mask2.view(torch.int32), mask.view(torch.int32))
        with pytest.raises(RuntimeError, match="bad argument"):
            _lib.call("mr_frames_to_batch_typed", _lib.ptr(frames), _lib.ptr(co), None, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0, _lib.ptr(work), wbytes,
                      _lib.ptr(img2), _lib.ptr(mask2), 3, N, Hs, Ws, H, W, _lib.stream_ptr(cuda), 3, _lib.DTYPE_F32)


# ---------------------------------------------------------------------------------------------------
# the fused pair path on a compact batch == the fp32 path on the widened batch
# ---------------------------------------------------------------------------------------------------


def _renderer(is_, dev):
    from handobjectconsist_amd.neurender.renderer import Renderer

    return Renderer(image_size=is_, R=torch.eye(3, device=dev)[None], t=torch.zeros(1, 3, device=dev), K=torch.ones(1, 3, 3, device=dev),
                    orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True, light_intensity_ambient=0.8)


def _pair(cuda, monkeypatch, B, is_, H, Wd, Cj, crit, use_backward, path, batch, seed, calls):
    """flow_pair_loss on (hand, object) parts along ``path`` -- "step" (the two struct calls), "node" (the node pair with the
    unit gradient) or "nograd" (the node pair's loss-only form under no_grad: validation) -- on ``batch``: the images and masks
    as [image_ref, image, jitter_ref, jitter] tensors of whatever types.  Poisoned scratch."""
    from handobjectconsist_amd.warping import opticalflow

    monkeypatch.setattr(opticalflow, "DEBUG_POISON_RENDER_OUTPUTS", True)
    monkeypatch.setattr(opticalflow, "USE_PAIR_STEP", path == "step")
    s = synth.random_scene(B, seed=seed, image_size=is_)
    hand_faces = t(s["hand_faces"].astype(np.int64), cuda)
    obj_faces = t(s["obj_faces"].astype(np.int64)[None].repeat(B, 0), cuda)
    leaves = [t(s[k], cuda).requires_grad_(path != "nograd") for k in ("hand_verts1", "obj_verts1", "hand_verts2", "obj_verts2")]
    wf, wb = torch.linspace(0.5, 1.5, B, device=cuda), torch.linspace(2.0, 0.25, B, device=cuda)
    ws = torch.linspace(-0.5, 0.75, B, device=cuda)
    del calls[:]
    with torch.set_grad_enabled(path != "nograd"):
        res = opticalflow.flow_pair_loss([(leaves[0], leaves[1]), (leaves[2], leaves[3])], (hand_faces, obj_faces),
                                         [t(s["K1"], cuda), t(s["K2"], cuda)], _renderer(is_, cuda), (Wd, H), *batch,
                                         ignore_face_idxs=synth.HAND_IGNORE_FACES, with_sum=True,
                                         with_mean="sum" if use_backward else "fwd", criterion=crit)
    assert res is not None, "the fused path must take this batch"
    lf, lb, flows, lsum, mean = res
    grads = None
    if path != "nograd":
        total = (lf * wf).sum() + (lb * wb).sum() + (lsum * ws).sum() + 3.0 * mean
        grads = torch.autograd.grad(total, leaves)
    base = flows[0]._base
    hit = base._hoc_coverage[0]
    words = hit.contiguous().view(torch.int32).view(2 * B, (is_ + 7) // 8, (is_ + 31) // 32).cpu().numpy() != 0
    yy, xx = np.mgrid[0:H, 0:Wd]
    defined = torch.from_numpy(words[:, (is_ - 1 - yy) >> 3, xx >> 5]).to(cuda)
    assert torch.isnan(base.detach()[~defined]).all(), "nothing is written under uncovered tiles"
    return (lf.detach(), lb.detach(), lsum.detach(), mean.detach().reshape(1), base.detach()[defined], hit.clone()), grads, list(calls)


# the shapes of test_gpu_warp.test_pair_step_equals_the_node_pair (without its camera variants) + one more non-square crop
SHAPES = [(3, 256, 256, 256, 3), (2, 96, 64, 80, 1), (1, 480, 270, 480, 3), (5, 128, 128, 128, 1), (3, 128, 128, 96, 3),
          (2, 256, 144, 256, 3)]


@pytest.mark.parametrize("crit_name", ["l1", "l2"])
@pytest.mark.parametrize("B,is_,H,Wd,Cj", SHAPES)
def test_compact_batch_equals_the_fp32_path_on_the_widened_batch(cuda, monkeypatch, B, is_, H, Wd, Cj, crit_name):
    """Per-sample losses (forward, backward, their sum), the batch mean, the flows under covered tiles and the coverage bytes
    bit for bit; vertex gradients at test_pair_step_equals_the_node_pair's tolerance for the same comparison (the scatter's
    flush uses fp32 global atomics).  l1 and l2; use_backward on and off; one- and three-channel masks; the struct path, the
    node pair and the node pair under no_grad; bf16 images with uint8 and with fp32 masks; poisoned scratch."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import opticalflow, pairstep

    crit = {"l1": _lib.CRITERION_L1, "l2": _lib.CRITERION_L2}[crit_name]
    calls = []
    real_call, real_step = _lib.call, pairstep.pair_step
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(pairstep, "pair_step", lambda *a, **k: (calls.append("pair_step"), real_step(*a, **k))[1])
    assert opticalflow.USE_UNIT_GRADIENT
    seed = 41 + B
    im_ref, im, jm_ref, jm = [t(a, cuda) for a in synth.random_images(B, H, Wd, seed + 1)]
    jm_ref, jm = jm_ref[:, :Cj].contiguous(), jm[:, :Cj].contiguous()
    im_ref16, im16 = im_ref.bfloat16(), im.bfloat16()
    assert not torch.equal(im16.float(), im), "the images must actually lose bits in bf16"
    batches = {"bf16/u8": [im_ref16, im16, jm_ref.to(U8), jm.to(U8)], "bf16/f32": [im_ref16, im16, jm_ref, jm]}
    widened = [im_ref16.float(), im16.float(), jm_ref, jm]
    for use_backward in (True, False):
        for path in ("step", "node", "nograd"):
            ref, ref_grads, ref_calls = _pair(cuda, monkeypatch, B, is_, H, Wd, Cj, crit, use_backward, path, widened, seed, calls)
            assert not any(c.endswith("_typed") for c in ref_calls)
            assert float(ref[0].abs().sum()) > 0 and float(ref[1].abs().sum()) > 0
            for kind, batch in batches.items():
                if kind == "bf16/f32" and not (use_backward and path != "node"):
                    continue  # (the second instantiation: once per launch form is enough)
                got, grads, got_calls = _pair(cuda, monkeypatch, B, is_, H, Wd, Cj, crit, use_backward, path, batch, seed, calls)
                where = (kind, path, use_backward)
                if path == "step":
                    assert "pair_step" in got_calls and not any(c.startswith("mr_flow_pair_forward") for c in got_calls), where
                    word = _lib.DTYPE_BF16 | ((_lib.DTYPE_U8 if kind == "bf16/u8" else _lib.DTYPE_F32) << 8)
                    assert any(p.st.reserved == word and p.st.criterion == crit for p in pairstep._PLANS.values()), where
                else:
                    want = "mr_flow_pair_forward_grad_tiles_typed" if path == "node" else "mr_flow_pair_forward_tiles_typed"
                    assert want in got_calls and "pair_step" not in got_calls, (where, got_calls)
                for x, y, what in zip(got, ref, ("loss_fwd", "loss_bwd", "loss_bwd + loss_fwd", "batch mean", "flows", "coverage bytes")):
                    assert torch.equal(x, y), (what, where)
                if grads is not None:
                    for x, y, what in zip(grads, ref_grads, ("hand 1", "object 1", "hand 2", "object 2")):
                        assert torch.isfinite(x).all() and float(y.abs().sum()) > 0, (what, where)
                        close(x.cpu().numpy(), y.cpu().numpy(), 1e-5, 1e-6 * float(y.abs().max()), f"d/d vertices of {what} {where}")


def test_compact_batch_and_the_recomputing_backward(cuda, monkeypatch):
    """mr_flow_pair_backward_tiles reads fp32 images: with USE_UNIT_GRADIENT off a compact batch is refused with an explicit
    error instead of being read as something it is not; under no_grad (nothing to differentiate) it still runs."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import opticalflow

    B, is_ = 2, 96
    monkeypatch.setattr(opticalflow, "USE_UNIT_GRADIENT", False)
    im_ref, im, jm_ref, jm = [t(a, cuda) for a in synth.random_images(B, is_, is_, 5)]
    batch = [im_ref.bfloat16(), im.bfloat16(), jm_ref.to(U8), jm.to(U8)]
    calls = []
    with pytest.raises(RuntimeError, match="recomputing backward"):
        _pair(cuda, monkeypatch, B, is_, is_, is_, 3, _lib.CRITERION_L1, True, "node", batch, 7, calls)
    got, _, _ = _pair(cuda, monkeypatch, B, is_, is_, is_, 3, _lib.CRITERION_L1, True, "nograd", batch, 7, calls)
    ref, _, _ = _pair(cuda, monkeypatch, B, is_, is_, is_, 3, _lib.CRITERION_L1, True, "nograd", [x.float() for x in batch], 7, calls)
    assert all(torch.equal(x, y) for x, y in zip(got, ref))


def test_pair_consist_upcasts_a_compact_batch_once(cuda):
    """imgflowarp.pair_consist (dense kernels, outputs="full") stays fp32: a compact batch gives what its .float() gives."""
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    B, H, W = 2, 48, 64
    rng = np.random.default_rng(4)
    flows = [t(rng.uniform(-3, 3, (B, H, W, 2)).astype(np.float32), cuda) for _ in range(2)]
    im_ref, im, jm_ref, jm = [t(a, cuda) for a in synth.random_images(B, H, W, 6)]
    compact = [im_ref.bfloat16(), im.bfloat16(), jm_ref.to(U8), jm.to(U8)]
    for outputs in ("full", "loss"):
        got = imgflowarp.pair_consist(flows, *compact, PyramidCriterion("l1"), use_backward=True, outputs=outputs)
        ref = imgflowarp.pair_consist(flows, *[x.float() for x in compact], PyramidCriterion("l1"), use_backward=True, outputs=outputs)
        assert torch.equal(got[0], ref[0]) and float(ref[0].abs().sum()) > 0
        if outputs == "full":
            assert torch.equal(got[2][0], ref[2][0]) and got[2][0].dtype == F32


# ---------------------------------------------------------------------------------------------------
# distance from the fp32 path / the reference on the metric scene: a derived bound
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("crit_name", ["l1", "l2"])
def test_compact_batch_stays_within_the_derived_bound_on_the_metric_scene(cuda, monkeypatch, crit_name):
    """tests/golden/chain_metric.npz's scene (the bench's meshes at 256 x 256; images normalised to [-0.5, 0.5]) with the fp32
    batch and with the same batch rounded to bf16 / converted to u8.

    Bound, l1.  Round-to-nearest-even to bf16 (8 significand bits) moves a value v by at most 2^-9 |v| <= 2^-10 for |v| <= 0.5,
    and keeps it in [-0.5, 0.5].  A warped value is a bilinear combination of four such values with non-negative weights
    summing to at most 1 (times a 0 / 1 mask), so it moves by at most 2^-10 as well; the target pixel moves by at most 2^-10.
    No mask depends on an image value (the u8 mask equals the fp32 mask where either is compared with 1), so both paths average
    over the SAME pixels.  Hence every term |warped - target| moves by at most 2^-9, and so does every per-sample masked mean.

    Bound, l2.  The term is res^2 with res = warped - target; |res| <= 1 on both paths (all values in [-0.5, 0.5]) and res
    moves by d, |d| <= 2^-9, so |res'^2 - res^2| = |d| |res' + res| <= 2 * 2^-9 per term, hence per masked mean.

    (fp32 rounding inside either path is five orders of magnitude below these bounds.)  Against the reference run's fixture
    (l1: wb_diff_losses = loss_bwd + loss_fwd per sample, which the fp32 path meets to 1e-5 relative --
    test_gpu_trainer.py): two directions' bounds plus that tolerance.

    Largest differences observed (MI355X): l1 2.5e-06 forward / 2.5e-06 backward (bound 1.95e-03); l2 1.4e-06 / 7.3e-07 (bound 3.91e-03); l1 per-sample loss sums through warpbranch.forward against the reference run's: 6.5e-06 compact, 3.0e-08 fp32 (bound 3.91e-03 + 1e-5 relative)."""
    from handobjectconsist_amd import _lib

    z = np.load(os.path.join(GOLDEN, "chain_metric.npz"))
    m = json.loads(str(z["meta"]))
    B, is_ = m["batch"], m["image_size"]
    crit = {"l1": _lib.CRITERION_L1, "l2": _lib.CRITERION_L2}[crit_name]
    bound = 2.0 ** -9 if crit_name == "l1" else 2.0 * 2.0 ** -9
    im_ref, im, jm_ref, jm = [t(a, cuda) for a in synth.random_images(B, is_, is_, m["scene_seed"])]
    assert float(im.abs().max()) <= 0.5 and float(im_ref.abs().max()) <= 0.5
    calls = []
    worst = [0.0, 0.0]
    for path in ("step", "nograd"):
        ref, _, _ = _pair(cuda, monkeypatch, B, is_, is_, is_, 3, crit, True, path, [im_ref, im, jm_ref, jm], m["scene_seed"], calls)
        got, _, _ = _pair(cuda, monkeypatch, B, is_, is_, is_, 3, crit, True, path,
                          [im_ref.bfloat16(), im.bfloat16(), jm_ref.to(U8), jm.to(U8)], m["scene_seed"], calls)
        assert torch.equal(got[5], ref[5]) and torch.equal(got[4], ref[4]), "flows and coverage do not depend on the images"
        assert float(ref[0].min()) > 0 and float(ref[1].min()) > 0
        for k in (0, 1):
            d = float((got[k].double() - ref[k].double()).abs().max())
            worst[k] = max(worst[k], d)
            print(f"compact vs fp32, {crit_name}, {path}, {('loss_fwd', 'loss_bwd')[k]}: max |difference| {d:.3e} (bound {bound:.3e})")
            assert d <= bound, (crit_name, path, k, d)
        assert not torch.equal(got[0], ref[0]), "the rounded images must actually change the loss"
    if crit_name == "l1":
        # ... and through warpbranch.forward as the trainer calls it, exactly as test_gpu_trainer.py runs the fixture's pair
        from handobjectconsist_amd.models import warpbranch
        from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
        from handobjectconsist_amd.neurender.renderer import Renderer

        s = synth.random_scene(B, seed=m["scene_seed"], image_size=is_)
        ren = Renderer(image_size=is_, R=torch.eye(3, device=cuda).unsqueeze(0), t=torch.zeros(1, 3, device=cuda),
                       K=torch.ones(1, 3, 3, device=cuda), orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True)
        want = z["wb_diff_losses"].astype(np.float64)
        for compact in (False, True):
            images = [x.bfloat16() if compact else x for x in (im, im_ref)]
            jitters = [x.to(U8) if compact else x for x in (jm, jm_ref)]
            samples, results = [], []
            for k in (0, 1):
                f = "12"[k]
                samples.append({"image": images[k], "jittermask": jitters[k], "camintr": t(s["K" + f], cuda),
                                "objfaces": t(s["obj_faces"][None].repeat(B, 0), cuda), "objverts3d": t(s["obj_verts" + f], cuda),
                                "handverts3d": t(s["hand_verts" + f], cuda)})
            results.append({"recov_handverts3d": t(s["hand_verts1"], cuda).requires_grad_(True),
                            "recov_objverts3d": t(s["obj_verts1"], cuda).requires_grad_(True)})
            results.append({"recov_handverts3d": t(z["pred1_hand"], cuda), "recov_objverts3d": t(z["pred1_obj"], cuda)})
            loss, pair = warpbranch.forward(samples, results, t(s["hand_faces"], cuda)[None], ren, (is_, is_), PyramidCriterion("l1"),
                                            gt_refs=True, first_only=True, hand_ignore_faces=m["hand_ignore_faces"],
                                            use_backward=True, pair_outputs="loss")
            d = np.abs(pair["diff_losses"].detach().double().cpu().numpy() - want).max()
            print(f"{'compact' if compact else 'fp32'} vs the reference's per-sample loss sums: max |difference| {d:.3e}")
            tol = (2 * bound if compact else 0.0) + 1e-5 * np.abs(want).max()
            assert d <= tol, (compact, d, tol)


# ---------------------------------------------------------------------------------------------------
# dataset -> training step
# ---------------------------------------------------------------------------------------------------


def test_dataset_to_training_step_on_a_compact_batch(cuda, monkeypatch):
    """HandObjSet -> seq_extend_collate -> assemble_batch(image_dtype=bfloat16, mask_dtype=uint8) -> WarpRegNet consistency
    step: the compact batch reaches the trunk and the struct path as it is, the step's loss and gradients are finite, and the
    pair loss of the step is, bit for bit, the one the struct path computes from the SAME predicted vertices and the widened
    batch (one pass through the network: the second ``pair_step`` call is made where the first one is, on its arguments).

    The dataset is built with ``center_idx=None``: the consistency term renders the annotated frame's vertices with that
    frame's intrinsics, so they have to be in the camera frame.  Centred on a joint (``center_idx=9``) they sit around
    z = 0, in front of the near plane, the annotated render covers nothing and the pair loss is exactly 0 for any image:
    a comparison of two zeros would show nothing, hence the ``> 0``."""
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.models.synthnet import SynthMeshRegNet
    from handobjectconsist_amd.models.warpreg import WarpRegNet
    from handobjectconsist_amd.utils import collate
    from handobjectconsist_amd.warping import pairstep

    res = (64, 64)
    ds = synthpose.SynthPoseDataset(3, frame_size=(320, 240), seed=4)
    hs = handobjset.HandObjSet(ds, inp_res=res, sample_nb=2, spacing=1, block_rot=True, sides="right", center_idx=None)
    torch.manual_seed(0)
    batch = collate.seq_extend_collate([hs[i] for i in (0, 2, 4)], ["objverts3d", "objfaces", "objcanverts"])
    plain = handobjset.assemble_batch(batch, cuda, res)
    samples = handobjset.assemble_batch(batch, cuda, res, image_dtype=BF16, mask_dtype=U8)
    for s, p in zip(samples, plain):
        assert s["image"].dtype == BF16 and s["jittermask"].dtype == U8
        assert torch.equal(s["image"], p["image"].bfloat16()) and torch.equal(s["jittermask"], (p["jittermask"] == 1).to(U8))
    seen, pairs = [], []
    real_step = pairstep.pair_step

    def both(*a, **k):
        seen.append(tuple(x.dtype for x in a[10:14]))
        # the widened batch on the same vertices, faces, cameras and renderer (its autograd node is simply dropped)
        wide = real_step(*a[:10], *[x.float() for x in a[10:14]], *a[14:], **k)
        got = real_step(*a, **k)
        pairs.append((got, wide))
        return got

    monkeypatch.setattr(pairstep, "pair_step", both)
    torch.manual_seed(0)
    model = SynthMeshRegNet().to(cuda).eval()
    trunk_saw = []
    real_encode = model.encode
    monkeypatch.setattr(model, "encode", lambda images: (trunk_saw.append(images.dtype), real_encode(images))[1])
    pre = WarpRegNet(res, model, lambda_consist=0.5, lambda_data=0.5, criterion="l1", gt_refs=True, use_backward=True,
                     mano_faces=model.mano_layer.th_faces, pair_outputs="loss").to(cuda)
    pre.step_count = 1000
    loss, losses, _, _ = pre({"data": samples, "supervision": "consist"})
    loss.backward()
    assert torch.isfinite(loss) and "warp_consist" in losses
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert trunk_saw and all(d == BF16 for d in trunk_saw), trunk_saw
    assert len(seen) == 1 and seen[0] == (BF16, BF16, U8, U8), seen
    got, wide = pairs[0]
    assert got is not None and wide is not None, "the struct path must take both batches"
    print(f"pair loss of the step: compact {float(got[0])!r}, widened {float(wide[0])!r}")
    assert float(wide[0]) > 0 and torch.equal(losses["warp_consist"].detach(), got[0].detach())
    for k, name in enumerate(("mean", "loss_sum", "loss_fwd", "loss_bwd")):
        assert torch.equal(got[k].detach(), wide[k].detach()), name
    assert torch.equal(got[5], wide[5]), "coverage"
