"""The frame-pair step at the borders of the image and the raster: tests/pair_border_cases.py's wall scenes -- every pixel
carries a flow, bilinear taps leave the image on all four sides, the outermost rows and columns hold valid loss samples (jitter
masks of ones), hundreds of vertices are off-screen and some of them carry a gradient, the occlusion step's nearest-neighbour
warp leaves the raster, faces cross the whole raster edge -- through ``opticalflow.flow_pair_loss`` on (hand, object) parts
against the CPU oracle, with the machinery, the checks and the rules of tests/test_gpu_pair_meshes.py
(tests/pair_oracle_harness.py), unchanged.  tests/test_pair_border_cases_host.py proves on the CPU, from the oracle alone, that
every case reaches every border class and that the fused path takes it.

    W1   B 4, raster 64, crop 64 x 64, wall 24 x 24   step (two calls through one plan), node pair, composed path
    W2   W1 at crop 45 x 52 (odd width)               step; compact batch (bf16 images, u8 masks) against the widened one
    W3   B 2, raster 96, crop 96 x 54                 per-sample camera, one-channel masks: step, node pair, l2
    W4   B 2, raster 64, wall 4 x 4 of 1.32 m         18 faces about 60 px across, |NDC| up to 3; crops 64 x 64 and 45 x 52
    W5   B 3, raster 64, left / top zero border       a frame moved off-screen in samples 0 and 1: loss and gradient exactly
                                                      zero, finite; sample 2 within the rules

Measured on the MI355X (256 compute units), the largest over both seeds and every path of the case, in units of the rule;
oracle seconds per seed on that machine's host, 8 threads.  Every non-zero pattern was exact, no seed was discarded.

    case  oracle s  flows    losses  gradients
    W1      0.2     < 0.001  0.001   0.006    (step, node pair and composed path)
    W2      0.2     < 0.001  0.001   0.008    (compact / widened batch: 0.001, 0.006)
    W3      0.2     < 0.001  0.001   0.006    (l2: losses 0.008, gradients 0.010)
    W4      0.1     < 0.001  0.001   0.007    (crop 64 x 64)
    W4c     0.1     < 0.001  0.001   0.005    (crop 45 x 52)
    W5      0.1     < 0.001  0.001   0.005    (samples 0 and 1: exactly zero)

No case exceeded the gradient rule, so no bound comes from the oracle's fp32 chain.  The whole file takes 5 s on the GPU.
"""
import pytest

from tests import pair_border_cases as PB
from tests.pair_oracle_harness import compact_case, composed_case, fused_case

pytestmark = pytest.mark.gpu

FUSED = list(PB.CASES)
NODE = [n for n, c in PB.CASES.items() if c["node"]]
assert FUSED == ["W1", "W2", "W3", "W4", "W4c", "W5"] and NODE == ["W1", "W3"]


@pytest.mark.parametrize("name", FUSED)
def test_pair_step_at_the_borders(cuda, monkeypatch, name):
    """the struct path (mr_pair_step_forward / _backward), two calls through one plan"""
    fused_case(cuda, monkeypatch, name, "step", zero_samples=PB.ZERO_SAMPLES.get(name, ()))


@pytest.mark.parametrize("name", NODE)
def test_node_pair_at_the_borders(cuda, monkeypatch, name):
    """USE_PAIR_STEP off: the node pair"""
    fused_case(cuda, monkeypatch, name, "node")


def test_l2_criterion_at_the_borders(cuda, monkeypatch):
    fused_case(cuda, monkeypatch, PB.L2_CASE, "step", crit="l2")


def test_compact_batch_at_the_borders(cuda, monkeypatch):
    """odd width: the rows of the bf16 and u8 planes start at odd elements"""
    assert PB.CASES[PB.COMPACT_CASE]["crop"][0] % 2 == 1
    compact_case(cuda, monkeypatch, PB.COMPACT_CASE)


def test_composed_path_at_the_borders(cuda, monkeypatch):
    """get_opticalflow + pair_consist (the dense kernels' path) on the same scene against the same oracle"""
    composed_case(cuda, monkeypatch, PB.COMPOSED_CASE, fused_takes_it=True)
