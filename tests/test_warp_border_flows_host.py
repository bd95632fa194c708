"""tests/warp_border_flows.py on the CPU: the flow fields of tests/test_gpu_warp_borders.py reach every border class on every
side, and the oracle those tests compare with (oracle/warp_ref.py) is torch's own ``grid_sample`` on these very flows --
bilinear and nearest, masks exactly, NaN patterns included, with NaN in the image's outer ring.

That comparison is what found the oracle multiplying a skipped tap by zero instead of skipping it: with a NaN at the clamped
address it gave NaN where ``grid_sample`` gives 0.  Where a flow component is +-inf or NaN the position is non-finite and
``grid_sample``'s answer is the float-to-int conversion's of the platform (NaN on this CPU); the oracle, like the kernels,
counts such a position as out of bounds: sample 0, mask 0.  That choice is asserted here so that it cannot drift."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import warp_ref as W
from tests import warp_border_flows as BF

SHAPES = [(64, 64), (52, 45), (7, 5), (2, 2)]
SEEDS = (3, 7, 8, 11, 12)  # the ones tests/test_gpu_warp_borders.py uses


def _torch_warp(x, flow, mode):
    """imgflowarp.warp as the reference writes it, on torch's CPU grid_sample"""
    xt, ft = torch.from_numpy(x), torch.from_numpy(flow)
    _, _, H, Wd = xt.shape
    xx = torch.arange(Wd).view(1, -1).repeat(H, 1)
    yy = torch.arange(H).view(-1, 1).repeat(1, Wd)
    vg = torch.stack([xx, yy], 0)[None].float() + ft
    vg = torch.stack([2.0 * vg[:, 0] / max(Wd - 1, 1) - 1.0, 2.0 * vg[:, 1] / max(H - 1, 1) - 1.0], 1).permute(0, 2, 3, 1)
    out = F.grid_sample(xt, vg, mode=mode, align_corners=False)
    mask = F.grid_sample(torch.ones_like(xt), vg, mode=mode, align_corners=False)
    mask[mask < 0.99999] = 0
    mask[mask > 0] = 1
    return (out * mask).numpy(), mask.numpy()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("H,Wd", SHAPES)
def test_every_class_on_every_side(H, Wd, seed):
    flow, reached = BF.border_flow(2, H, Wd, seed)
    counts = BF.check_classes(flow, reached, all_on_every_side=min(H, Wd) >= 5)
    assert flow.dtype == np.float32 and flow.shape == (2, 2, H, Wd)
    if (H, Wd) == (64, 64):  # (the only width at which fp32 reaches the first pixel centre exactly)
        assert all(b == 0 for s in BF.SIDES for (_, _, _, b) in reached[(s, "on")])
    print(f"{H}x{Wd} seed {seed}: at least {min(counts.values())} pixels per reached (side, class)")


@pytest.mark.parametrize("nan_ring", [False, True])
@pytest.mark.parametrize("H,Wd", SHAPES)
def test_the_oracle_is_grid_sample_on_these_flows(H, Wd, nan_ring):
    flow, _ = BF.border_flow(2, H, Wd, 3)
    x = np.random.default_rng(5).uniform(-0.5, 0.5, (2, 3, H, Wd)).astype(np.float32)
    if nan_ring:
        x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = np.nan, np.nan, np.nan, np.nan
    finite = np.broadcast_to(np.isfinite(flow).all(1)[:, None], x.shape)
    assert (~finite).any() and finite.any()
    for mode in ("bilinear", "nearest"):
        out, mask = W.warp(x, flow, mode=mode)
        t_out, t_mask = _torch_warp(x, flow, mode)
        assert (mask[finite] == t_mask[finite]).all(), mode
        assert (np.isnan(out) == np.isnan(t_out))[finite].all(), mode
        ok = finite & ~np.isnan(out)
        assert (np.abs(out - t_out)[ok] <= 2e-6 + 1e-5 * np.abs(t_out[ok])).all(), mode
        if nan_ring and min(H, Wd) > 2:  # (2 x 2 is all ring)
            assert np.isnan(out[finite]).any() and (mask[finite] == 1).any()
        # a non-finite position is out of bounds
        assert (out[~finite] == 0).all() and (mask[~finite] == 0).all(), mode
