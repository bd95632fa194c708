"""The upstream gradients the pair step's backward is tested over, and the wall scenes whose images cover enough tiles for the
backward scatter's fixed point to give up bits (a helper module: nothing pytest collects).

``SPECS``: name -> ``spec(B)``, an ``pair_oracle_harness.Upstream``.  Every per-sample coefficient -- ``wf + ws + wm / B`` for
loss_fwd, ``wb + ws + wm / B`` for loss_bwd, absent terms left out -- is EXACT in fp32 in whatever order its terms are added:
the values are signed powers of two with a few mantissa bits and ``wm`` is a multiple of B.  The device, torch's autograd on the
node path and the oracle each add in an order of their own; with exact sums a test measures the kernels, not that order.
tests/test_pair_upstream_cases_host.py checks the exactness of every spec at every batch size it is used at.

``CASES``: ``pair_border_cases``' wall scenes at the smallest rasters (multiples of 4, as the fused path's gate asks) at which
a workgroup of ``unit_scatter_tiles_kernel`` reaches ``headroom`` 1 and 2: the same host test proves both with
tests/host/launch_plan_cases.cpp on the oracle's coverage, and that no other case of the suite reaches either.
"""
import numpy as np

from tests import pair_border_cases as PB

P2 = lambda e: float(2.0 ** e)


def _take(values, B):
    assert B <= len(values)
    return np.array(values[:B], np.float32)


_WF, _WB, _WS = (1.5, -0.75, 2.0, 0.5), (-1.25, 3.0, 0.375, -2.0), (0.5, 1.0, -0.25, 1.5)
_WM_SHARE = -3.0  # every sample's share of the mean's weight: wm = -3 B


def _subset(parts, with_mean):
    def spec(B):
        from tests.pair_oracle_harness import Upstream

        return Upstream(wf=_take(_WF, B) if "fwd" in parts else None, wb=_take(_WB, B) if "bwd" in parts else None,
                        ws=_take(_WS, B) if "sum" in parts else None, wm=_WM_SHARE * B if "mean" in parts else None, with_mean=with_mean)
    return spec


def _plain(wf, wb, ws=None, wm_share=None, with_mean="sum"):
    def spec(B):
        from tests.pair_oracle_harness import Upstream

        return Upstream(wf=_take(wf, B), wb=_take(wb, B), ws=None if ws is None else _take(ws, B),
                        wm=None if wm_share is None else wm_share * B, with_mean=with_mean)
    return spec


# the subsets of the four outputs a loss may use (part a): name -> the outputs in the loss
SUBSETS = {"fwd": ("fwd",), "bwd": ("bwd",), "sum": ("sum",), "mean": ("mean",), "fwd+bwd": ("fwd", "bwd"), "bwd+mean": ("bwd", "mean"),
           "sum+mean": ("sum", "mean"), "all": ("fwd", "bwd", "sum", "mean")}
INF, NAN = float("inf"), float("nan")

SPECS = {
    **{f"{k}/{m}": _subset(v, m) for k, v in SUBSETS.items() for m in ("sum", "fwd")},
    # magnitudes 2^-100 .. 2^100 and both signs across the samples of one call; sample 2: both coefficients zero by absence
    # (nothing but a zero weight); sample 3: loss_fwd's coefficient zero, loss_bwd's not
    "spread": _plain((P2(100), -1.5 * P2(-100), 0.0, 0.0), (-1.75 * P2(-100), 1.25 * P2(100), 0.0, -1.5 * P2(37))),
    # sample 1: both coefficients cancel, -3.5 + 1.5 + 2 == 0, every term non-zero; sample 3: loss_bwd's alone, -3 + 1 + 2 == 0
    "cancel": _plain((1.5, -3.5, 1.0, 0.5), (-1.25, -3.5, 2.0, -3.0), ws=(0.5, 1.5, -0.25, 1.0), wm_share=2.0),
    # sample 1: 2^-140, an fp32 denormal; its gradients leave the normal range
    "denormal": _plain((1.5, P2(-140), -0.75, 2.0), (-1.25, P2(-140), 3.0, 0.5)),
    "inf": _plain((1.5, INF, -0.75, 2.0), (-1.25, 3.0, 0.375, -2.0)),
    "nan": _plain((1.5, -0.75, 2.0, 0.5), (-1.25, 3.0, NAN, -2.0)),
    # the second backward through one forward (part g): other signs, other magnitudes, sample 1 zero
    "second": _plain((-P2(20), 0.0, 1.5 * P2(-30), -3.0), (P2(-20), 0.0, -P2(10), 0.75)),
}
ZERO_GRAD_SAMPLES = {"spread": (2,), "cancel": (1,), "second": (1,)}  # samples whose two coefficients are both exactly zero
LOSS_SCALE = P2(16)
# (spec, batch sizes it is used at): what the host test checks for exactness
USED_AT = {**{k: (4, 3) for k in SPECS}, "spread": (4, 3, 2), "cancel": (4,), "denormal": (4,), "inf": (4,), "nan": (4,), "second": (4,)}

_T2, _TH2 = PB._T4[:2], (0.05, -0.04)
# Seeds: chosen so that the flows' non-zero pattern on the device equals the oracle's exactly; a case whose pattern differs FAILS.
CASES = {
    "X1": PB._case(2, 132, None, 24, _T2, _TH2, 31, note="raster 132 (4 x 17 tiles, the last row of tiles 4 rows high): headroom 1"),
    "X2": PB._case(2, 196, None, 24, _T2, _TH2, 31, note="raster 196 (7 x 25 tiles): headroom 2"),
}
HEADROOM = {"X1": 1, "X2": 2}
for _c in CASES.values():
    _c["tag"] = "PAIR-UPSTREAM"


def covered_tiles(fwd, raster):
    """the count of covered 32 x 8 tiles of every image of the stack (frame 1's B images, then frame 2's), from the oracle's
    face index maps (raster orientation: the rows the device's tiles are cut from)"""
    out = []
    for ro in fwd["renders"]:
        fim = ro["_saved"]["face_index_map"]
        assert fim.shape[1:] == (raster, raster)
        ty, tx = (raster + 7) // 8, (raster + 31) // 32
        pad = np.full((fim.shape[0], ty * 8, tx * 32), -1, fim.dtype)
        pad[:, :raster, :raster] = fim
        out.extend(int(n) for n in (pad.reshape(-1, ty, 8, tx, 32) >= 0).any(axis=(2, 4)).reshape(fim.shape[0], -1).sum(1))
    return out
