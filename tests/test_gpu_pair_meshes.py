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

What these scenes do NOT reach: every mesh sits in the middle of the raster and every jitter mask has a zero border, so no warp
sample has a tap beyond the image, no valid loss sample lies in an outermost row or column and no vertex is off-screen.  Those
classes are tests/test_gpu_pair_borders.py's.  The oracle, ``Run`` and the checks live in tests/pair_oracle_harness.py, shared
with that file.
"""
import pytest

from tests import pair_mesh_cases as P
from tests.pair_oracle_harness import FP32_CHAIN, compact_case, composed_case, fused_case  # noqa: F401 (FP32_CHAIN: the docstring's table)

pytestmark = pytest.mark.gpu


def _fused_case(cuda, monkeypatch, name, path, crit="l1"):
    fused_case(cuda, monkeypatch, name, path, crit)


def _composed_case(cuda, monkeypatch, name):
    composed_case(cuda, monkeypatch, name)


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
    compact_case(cuda, monkeypatch, P.COMPACT_CASE)


def test_composed_path_past_the_vertex_limit(cuda, monkeypatch):
    """V = 2561: flow_pair_loss returns None; get_opticalflow + pair_consist (mr_render_flow_backward answers NOTIMPL, the
    vertex-colour backward takes its gather) meet the same assertions against the same oracle"""
    _composed_case(cuda, monkeypatch, "K")


def test_objectless_pair_takes_the_composed_path(cuda, monkeypatch):
    """no object vertices: pair_step and flow_pair_loss answer None as for every other unsupported shape (they used to raise),
    and the composed path on the hand alone gives the oracle's results"""
    _composed_case(cuda, monkeypatch, "L")
