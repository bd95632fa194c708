"""The dense warp kernels with samples ON and AROUND the image border: mr_warp_forward / _backward (bilinear and nearest),
mr_occlusion_mask and mr_pair_consist_forward / _backward with their l2 forms, through ``imgflowarp.warp``,
``imgflowarp.get_occlusion_mask`` and ``imgflowarp.pair_consist``, on tests/warp_border_flows.py's flow fields: every pixel of
the outer two rows and columns sits, per side and corner, exactly on the first / last pixel centre, just inside or just outside
the 0.99999 validity band, half a pixel, one and three pixels out, or has a +-1e9, +-inf or NaN flow component; interior pixels
carry random flows.  These are the positions at which csrc/warp_device.hpp's border code decides a result -- ``inb``'s
comparisons, ``pair_addr``'s shifted row pairs and ``quad_of``'s selects, the clamped addresses, ``valid_mask`` at its
threshold -- and which random floats never reach.  Each test asserts on the CPU that every class is present on every side
before it launches anything (2 x 2 has 8 pixels for 36 side-class pairs: every class somewhere, every pixel a class).

Against the oracle (W.warp, W.warp_backward, W.get_occlusion_mask, W.pair_consist, W.pair_consist_grad; pinned to torch's
grid_sample on these very flows in tests/test_warp_border_flows_host.py):
    masks (warp, occlusion, full / warp / flow masks of the pair)   exact
    warp output                  1e-5 relative + 2e-6     (test_warp_golden)
    warp gradients               1e-4 relative + 1e-5     (test_warp_golden)
    pair losses                  1e-5 relative + 1e-7     (test_pair_consist_large_matches_oracle)
    pair flow gradients          1e-4 relative + 1e-9, element by element   (test_pair_consist_large_matches_oracle)
NaN patterns are compared as well: with NaN in the image's outer ring a tap the reference skips must not leak 0 x NaN, and
a tap it uses with weight 0 propagates it.  (The pair loss is not run on such images: the reference's masked mean multiplies
every pixel's difference by its mask, so one NaN pixel makes the loss NaN whatever the flows are.)

Inputs and outputs live in tests/guarded_alloc.py's guarded storage and the bands are checked.

Measured on the MI355X: every mask exact; warp outputs and gradients, pair losses and flow gradients at 0.01 of their rules
and less.  What the classes are worth, on scratch builds of warp_device.hpp with one value changed (never an address): the
validity threshold 5e-6 lower turns 15 of this file's 24 tests red and none of test_gpu_warp.py, test_gpu_pair_meshes.py and
test_gpu_fuzz.py; round-half-up instead of rintf in ``nearest_idx`` turns 5 red here (2 there).  The whole file takes 5 s.
"""
import numpy as np
import pytest
import torch

from handobjectconsist_amd.utils import synth
from oracle import warp_ref as W
from tests import guarded_alloc as G
from tests import warp_border_flows as BF

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (52, 45), (7, 5), (2, 2)]  # (H, W)
B = 2


def _flows(H, Wd, seed):
    flow, reached = BF.border_flow(B, H, Wd, seed)
    counts = BF.check_classes(flow, reached, all_on_every_side=min(H, Wd) >= 5)
    return flow, counts


def _close(got, ref, rtol, atol, what):
    """NaN and inf patterns equal, finite values within atol + rtol |ref|; returns the largest error in units of the rule"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert (np.isnan(got) == np.isnan(ref)).all(), \
        f"{what}: NaN pattern differs at {int((np.isnan(got) != np.isnan(ref)).sum())} elements ({int(np.isnan(ref).sum())} NaN in the oracle)"
    fin = np.isfinite(ref)
    assert (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all(), f"{what}: infinities differ"
    err, tol = np.abs(got - ref)[fin], (atol + rtol * np.abs(ref))[fin]
    units = float((err / tol).max()) if err.size else 0.0
    assert units <= 1.0, f"{what}: max err {err.max():.3e}, {(err > tol).sum()} / {err.size} out of tolerance ({units:.2f} of the rule)"
    return units


class _Guarded:
    def __init__(self, cuda, monkeypatch):
        self.cuda = cuda
        self.alloc = G.GuardedAllocator(cuda)
        self.alloc.install(monkeypatch)

    def up(self, a, grad=False):
        with self.alloc.paused():
            x = torch.from_numpy(np.ascontiguousarray(a)).to(self.cuda).clone()
        x = self.alloc.guard(x)
        return x.requires_grad_(True) if grad else x

    def close(self):
        damage = self.alloc.check()
        self.alloc.uninstall()
        assert not damage, "\n".join(damage)


def _image(H, Wd, seed, nan_ring):
    x = np.random.default_rng(seed).uniform(-0.5, 0.5, (B, 3, H, Wd)).astype(np.float32)
    if nan_ring:
        x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = np.nan, np.nan, np.nan, np.nan
    return x


@pytest.mark.parametrize("nan_ring", [False, True], ids=["plain", "nan-ring"])
@pytest.mark.parametrize("H,Wd", SHAPES)
def test_warp_at_the_borders(cuda, monkeypatch, H, Wd, nan_ring):
    from handobjectconsist_amd.warping import imgflowarp

    flow, counts = _flows(H, Wd, 3)
    x = _image(H, Wd, 5, nan_ring)
    grad_out = np.random.default_rng(6).standard_normal((B, 3, H, Wd)).astype(np.float32)
    g = _Guarded(cuda, monkeypatch)
    try:
        for mode in ("bilinear", "nearest"):
            ref_out, ref_mask = W.warp(x, flow, mode=mode)
            xt, ft = g.up(x, grad=True), g.up(flow, grad=True)
            out, mask = imgflowarp.warp(xt, ft, mode=mode)
            got_mask = mask.cpu().numpy()
            assert np.isfinite(got_mask).all() and np.isfinite(ref_mask).all()
            assert (got_mask != ref_mask).sum() == 0, f"warp mask {mode}: {int((got_mask != ref_mask).sum())} pixels differ"
            u = _close(out.detach().cpu().numpy(), ref_out, 1e-5, 2e-6, f"warp {mode}")
            print(f"WARP-BORDERS {H}x{Wd} {'nan-ring' if nan_ring else 'plain'} {mode}: output {u:.3f} of the rule; "
                  f"{int(ref_mask[:, 0].sum())} of {ref_mask[:, 0].size} samples valid; at least {min(counts.values())} pixels per class and side")
            if mode == "bilinear" and not nan_ring:
                (out * g.up(grad_out)).sum().backward()
                ref_gflow, ref_gx = W.warp_backward(x, flow, grad_out)
                ux = _close(xt.grad.cpu().numpy(), ref_gx, 1e-4, 1e-5, "grad_x")
                uf = _close(ft.grad.cpu().numpy(), ref_gflow, 1e-4, 1e-5, "grad_flow")
                print(f"WARP-BORDERS {H}x{Wd} bilinear: grad_x {ux:.3f}, grad_flow {uf:.3f} of the rule")
        assert (ref_mask == 0).any() and ((ref_mask == 1).any() or min(H, Wd) == 2)  # (2 x 2: every pixel a corner, none valid)
    finally:
        g.close()


@pytest.mark.parametrize("H,Wd", SHAPES)
def test_occlusion_mask_at_the_borders(cuda, monkeypatch, H, Wd):
    """four chained nearest-neighbour warps whose samples sit on the rounding half-way points and beyond every side; the masks
    take the values 0, 0.5 and 1 (a rendered alpha is not binary), whose products are exact in any order"""
    from handobjectconsist_amd.warping import imgflowarp

    f12, _ = _flows(H, Wd, 7)
    f21, _ = _flows(H, Wd, 8)
    rng = np.random.default_rng(9)
    m1 = (rng.random((B, 1, H, Wd)) < 0.85).astype(np.float32)
    m2 = rng.choice(np.array([0, 0.5, 1, 1, 1, 1], np.float32), (B, 1, H, Wd))
    f12_3 = np.concatenate([f12, np.ones((B, 1, H, Wd), np.float32)], 1)  # (flows arrive with a third channel)
    f21_3 = np.concatenate([f21, np.ones((B, 1, H, Wd), np.float32)], 1)
    ref1, ref2 = W.get_occlusion_mask(m1, m2, f12_3, f21_3)
    g = _Guarded(cuda, monkeypatch)
    try:
        o1, o2 = imgflowarp.get_occlusion_mask(g.up(m1), g.up(m2), g.up(f12_3), g.up(f21_3))
        for got, ref, what in ((o1, ref1, "occl1"), (o2, ref2, "occl2")):
            got = got.cpu().numpy()
            assert np.isfinite(got).all() and np.isfinite(ref).all()
            assert (got != ref).sum() == 0, f"{what}: {int((got != ref).sum())} of {ref.size} pixels differ"
        print(f"WARP-BORDERS {H}x{Wd} occlusion: {int((ref1 != 0).sum())} + {int((ref2 != 0).sum())} of {ref1.size} pixels pass the check")
    finally:
        g.close()


def _jitter(H, Wd, kind):
    jm = np.ones((2, B, 3, H, Wd), np.float32)
    if kind == "LT":
        jm[..., :, 0] = 0
        jm[..., 0, :] = 0
    return jm[0], jm[1]


@pytest.mark.parametrize("crit,jitter", [("l1", "ones"), ("l1", "LT"), ("l2", "ones")])
@pytest.mark.parametrize("H,Wd", SHAPES)
def test_pair_consist_at_the_borders(cuda, monkeypatch, H, Wd, crit, jitter):
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    flows = [np.ascontiguousarray(_flows(H, Wd, s)[0].transpose(0, 2, 3, 1)) for s in (11, 12)]
    im_ref, im, _, _ = synth.random_images(B, H, Wd, 13)
    jm_ref, jm = _jitter(H, Wd, jitter)
    gl = np.array([0.75, 1.5], np.float32)
    ref_loss, ref_masks, ref_warps, _, _ = W.pair_consist(flows, im_ref, im, jm_ref, jm, True, criterion=crit)
    ref_g = W.pair_consist_grad(flows, im_ref, im, jm_ref, jm, gl, True, criterion=crit)
    valid = [int(m["full_mask"].sum()) for m in ref_masks]
    if H * Wd > 4 and jitter == "ones":
        assert min(valid) > 0, valid
    g = _Guarded(cuda, monkeypatch)
    try:
        f12, f21 = g.up(flows[0], grad=True), g.up(flows[1], grad=True)
        loss, masks, warps, _ = imgflowarp.pair_consist([f12, f21], g.up(im_ref), g.up(im), g.up(jm_ref), g.up(jm), PyramidCriterion(crit),
                                                        use_backward=True, outputs="full")
        for i in (0, 1):
            for key in ("full_mask", "warp_mask", "flow_mask"):
                got, ref = masks[i][key].cpu().numpy(), ref_masks[i][key]
                assert (got != ref).sum() == 0, f"{key} {i}: {int((got != ref).sum())} elements differ"
            _close(warps[i].cpu().numpy(), ref_warps[i], 1e-5, 2e-6, f"warp {i}")
        ul = _close(loss.detach().cpu().numpy(), ref_loss, 1e-5, 1e-7, "loss")
        (loss * g.up(gl)).sum().backward()
        u12 = _close(f12.grad.cpu().numpy(), ref_g[0], 1e-4, 1e-9, "grad_flow12")
        u21 = _close(f21.grad.cpu().numpy(), ref_g[1], 1e-4, 1e-9, "grad_flow21")
        print(f"WARP-BORDERS {H}x{Wd} pair {crit} {jitter}: loss {ul:.3f}, flow gradients {max(u12, u21):.3f} of their rules; valid samples {valid}")
        # ... and without the per-pixel outputs (the same kernels with their debug stores off)
        f12b, f21b = g.up(flows[0], grad=True), g.up(flows[1], grad=True)
        loss_b = imgflowarp.pair_consist([f12b, f21b], g.up(im_ref), g.up(im), g.up(jm_ref), g.up(jm), PyramidCriterion(crit),
                                         use_backward=True, outputs="loss")[0]
        _close(loss_b.detach().cpu().numpy(), ref_loss, 1e-5, 1e-7, "loss (outputs='loss')")
        (loss_b * g.up(gl)).sum().backward()
        _close(f12b.grad.cpu().numpy(), ref_g[0], 1e-4, 1e-9, "grad_flow12 (outputs='loss')")
        _close(f21b.grad.cpu().numpy(), ref_g[1], 1e-4, 1e-9, "grad_flow21 (outputs='loss')")
    finally:
        g.close()
