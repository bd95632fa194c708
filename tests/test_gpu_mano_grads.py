"""mr_mano_forward / _backward and mr_mano_forward_full / _backward_full (csrc/mano_lbs.hip), EVERY component of grad pose,
grad betas and grad trans of every sample against the float64 central differences of oracle/mano_ref.py
(oracle/geom_grad_ref.py), normalised by that sample's largest reference gradient in that tensor -- where the directional
tests of test_gpu_warp.py / test_gpu_mano_full.py see one scalar per batch.  Values likewise, against the fp64 oracle.

Cases (tests/geom_grad_cases.py): the six variants of test_gpu_mano_full.VARIANTS through ``forward_full``, ``forward`` with
centre 9 and without a centre, an all-zero translation; B = 1 (twice), 32 (one full batch tile of the blend kernels) and 33;
sample 0 with a zero root rotation, sample 1 with (1e-6, 0, 0), sample 2 with 3.1 rad; six weight patterns on the outputs.

Tolerance: four times the error of the fp32 torch restatement on the CPU (``forward_torch``) in the same case and
tensor; tests/test_geom_grad_ref_host.py holds that yardstick to 2.5e-6 (gradients) / 1e-6 (values) and the differences to
1e-7 between eps and 10 eps.  Every case prints ``tensor yardstick/kernel`` on one line (profiles/geometry_grads.txt).

Measured on an MI355X (host: EPYC 9575F), largest kernel / yardstick ratio per tensor: verts 1.23, joints 1.24, grad pose
1.91, grad betas 2.15, grad trans 1.26.  The largest kernel error of any tensor is 2.19e-6 (grad pose, tip centre 20, B = 33,
where the yardstick reads 2.10e-6).

These tests found ``mano_pre_bwd_kernel`` and ``mano_skin_bwd_kernel`` accumulating their adjoints in fp32: grad betas was 5 to
11 fp32 ulps off (B = 1, zero root, tip weights: yardstick 9.30e-8, kernel 4.38e-7 = 4.71 x; tip centre 8: 7.22e-8 / 2.94e-7) and
grad trans under dense weights 7.67 x (6.45e-8 / 4.95e-7).  With those sums in double the same cases read 9.30e-8 / 9.30e-8,
7.22e-8 / 1.52e-7 and 6.45e-8 / 4.88e-8."""
import functools

import pytest
import torch

from tests import geom_grad_cases as C

pytestmark = pytest.mark.gpu

CASES = [(v, r, w) for v in C.MANO_VARIANTS for r in C.MANO_RUNS for w in C.MANO_WEIGHTS]  # (variant outermost: one reference each)


@functools.lru_cache(maxsize=None)
def layers(variant, device):
    """the layer on the GPU and, for the yardstick, on the CPU"""
    return C.make_layer(variant).to(device), C.make_layer(variant)


def test_the_variants_are_those_of_the_directional_tests():
    from tests import test_gpu_mano_full

    full = [v[1:4] + (v[4] == "given",) for v in C.MANO_VARIANTS.values() if v[0] == "forward_full" and v[4] != "zeros"]
    assert full == test_gpu_mano_full.VARIANTS


@pytest.mark.parametrize("variant,run,pattern", CASES, ids=["-".join(c) for c in CASES])
def test_every_gradient_component_matches_the_fp64_differences(cuda, variant, run, pattern):
    gpu_layer, cpu_layer = layers(variant, cuda)
    pose, betas, trans, wv, wj, ref = C.mano_case(variant, run, pattern)
    entry = C.MANO_VARIANTS[variant][0]
    raw = C.mano_run(gpu_layer, entry, pose, betas, trans, wv, wj)
    got, yard = C.as_f64(raw), C.as_f64(C.mano_run(cpu_layer, entry, pose, betas, trans, wv, wj))
    assert all(t.is_cuda and t.dtype == torch.float32 for t in raw.values())
    assert got["pose"].shape == tuple(pose.shape) and got["betas"].shape == tuple(betas.shape)
    report = C.Report(f"mano {variant} {run} {pattern}")
    for name in ("verts", "joints"):
        report.add(name, got[name], yard[name], ref[name], C.MAX_EY_VALUE)
    for name in ("pose", "betas", "trans"):
        if name in got:
            report.add("grad " + name, got[name], yard[name], ref[name], C.MAX_EY_GRAD)
    report.finish()
    if pattern == "zero" or C.MANO_VARIANTS[variant][4] == "zeros":  # exact zeros, and none of them negative
        for name in (("pose", "betas", "trans") if pattern == "zero" else ("trans",)):
            if name in raw:
                assert not bool((raw[name] != 0).any()) and not bool(torch.signbit(raw[name]).any()), name


@pytest.mark.parametrize("variant", ["forward-pca-centre9", "forward-pca-uncentred"])
@pytest.mark.parametrize("run", list(C.MANO_RUNS))
def test_the_two_entry_points_give_the_same_bits_where_both_apply(cuda, variant, run):
    """PCA coefficients, an articulated centre or none, no translation: ``forward`` and ``forward_full`` reach the same kernels
    through two entry-point pairs (mr_mano_forward / _backward with an empty ``ManoFull`` and a workspace without ``tflag``,
    mr_mano_forward_full / _backward_full) -- values and gradients bit for bit, under every weight pattern."""
    gpu_layer, _ = layers(variant, cuda)
    for pattern in C.MANO_WEIGHTS:
        pose, betas, trans, wv, wj = C.mano_case_inputs(variant, run, pattern)
        a = C.mano_run(gpu_layer, "forward", pose, betas, trans, wv, wj)
        b = C.mano_run(gpu_layer, "forward_full", pose, betas, trans, wv, wj)
        for name in a:
            assert torch.equal(a[name], b[name]), (pattern, name)
