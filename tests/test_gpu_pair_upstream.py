"""The frame-pair step's backward over the domain of its UPSTREAM gradient.  tests/test_gpu_pair_meshes.py and
tests/test_gpu_pair_borders.py vary the geometry under one fixed loss (all four outputs, O(1) weights, none zero); here the
geometry is W1 (B 4, raster 64), I (B 3, raster 96) and two wall scenes, and the loss varies: which of loss_fwd / loss_bwd /
their sum / the batch mean it uses, the coefficients' magnitudes (2^-140 .. 2^100, inf, NaN), signs and exact zeros, which
leaves want a gradient, a second backward through one forward.  Machinery, checks and rules are tests/pair_oracle_harness.py's,
unchanged: guarded inputs, poisoned outputs, the float64 oracle element by element, |got - ref| <= 1e-4 |ref| + 1e-5 x the
largest |ref| of the same sample and leaf -- a rule relative to the sample, so it holds at any coefficient in fp32's normal
range.  Specs and cases: tests/pair_upstream_cases.py; their exactness and the headroom proofs: tests/test_pair_upstream_cases_host.py.

What the backward does with the upstream (raster_bwd_vc.hip: st_unit_scalars and st_unit_coef, the coefficient phase of
scatter_tiles_body; the shift: launch_plan.hpp's st_headroom and st_shift): one coefficient per image,
(gl_dir + gl_sum + gl_mean / B) / count from the arrays present; a zero coefficient returns early; the fixed point's shift is
taken from the exponent of fl(unit_max x coefficient); a non-finite product switches the workgroup to fp32 global atomics; the
shift gives up one bit per doubling beyond 2^13 terms per table cell (``headroom``).

X1 (raster 132) and X2 (raster 196) are the smallest rasters at which every workgroup sums with headroom 1 and 2: at
headroom h a term is rounded to 2^-(37 - h) of fl(unit_max x coefficient)'s binade, and a vertex receives at most 768 x 25
terms, so the fixed point adds at most 19200 x 2^-35 = 5.6e-7 of the image's LARGEST PIXEL gradient to a vertex sum at
headroom 2 -- a derivation from the kernel's own statement, beside the oracle comparison below, not instead of it.

Found by this file: ``launch_unit_scatter_tiles`` demanded ``grad_loss_fwd || grad_loss_sum || grad_mean`` although
``mr_pair_step_backward`` accepts a call with ``grad_loss_bwd`` alone, so a loss that used loss_bwd only ended in
"mr_pair_step_backward failed: -1" on the step path (the node path passes zeros for an absent grad_loss_fwd).  The kernels read
every gl_* behind a null check; the launcher now accepts any of the four.

No test before this file reached the ``finite == false`` path: every upstream weight of the pair tests is O(1) and the unit
gradient's bound is finite, so fl(unit_max x coefficient) never left the normal range.

Measured on the MI355X (256 compute units), gradients in units of the rule, the largest over the four leaves; flows agreed to
better than 0.001 of their rule, losses to 0.001, every non-zero pattern was exact, no seed was discarded.  87 tests, 8 s for
the whole file (slowest: 1.3 s, the first test, which loads the library, and X2 through two seeds).

    a. subsets (8 x mean over sum / fwd), W1 and I, step and node   W1 0.019, I 0.012 (step and node pair alike); ``bwd`` alone
                                                                     raised "mr_pair_step_backward failed: -1" on the step path
                                                                     before the fix (4 of the 64 cases), passes since
       no output in the loss                                         every leaf None, nothing launched, nothing failed
    b. spread 2^-100 .. 2^100, cancel                                within a's figures; zero samples exactly zero
       loss scaler 2^16                                              0.008 both calls; scaled against 2^16 x unscaled: 0.000
    c. 2^-140                                                        other samples 0.005; the sample itself: all zeros, |ref| <= 2.0e-44
    d. +inf / NaN                                                    other samples 0.006 / 0.007; 1794 / 1800 elements per frame that
                                                                     the oracle has non-zero, none of them finite on the device
    e. headroom 1 (X1) / 2 (X2), default weights and spread          X1 0.007 / 0.007, X2 0.007 / 0.007; the device's covered-tile
                                                                     counts are the oracle's (85 and 175 per image: every tile)
    f. which leaves want a gradient, step and node                   0.008 (all four), 0.006, 0.005, 0.008; the others None
    g. two backwards through one forward                             0.008, then 0.006; the second's zero sample exactly zero

The denormal end.  torch hands the 2^-140 weight to the node as it is (7.175e-43); the kernel's coefficient is that over the
sample's count of valid loss terms (10449): 6.9e-47, below 2^-149 = 1.4e-45, the smallest fp32 denormal: it rounds to zero whether or not
denormals are kept, the image returns early, and the sample's gradient is the forward's zeros -- within 2e-44 of the oracle,
1.7e-6 of the 2^-126 allowed.  So this test cannot tell kept denormals from flushed ones at the issue's 2^-140; it pins that
nothing non-finite or large comes of an underflowing coefficient.

The headroom's other side.  ``terms`` counts three per pixel; a rasterised face gives a table cell one, and a workgroup walks
at most 27 tiles = 6912 pixels up to raster 320, fewer than the 2^13 the sums' field holds at headroom 0: leaving ``headroom``
out of ``shift`` changes no value here (measured: that mutant passes every test of this file).  What X1 and X2 pin is that the
bits given up are not missed: with twelve bits per step instead of one, X2 fails at 44 and 61 times the rule.
"""
import numpy as np
import pytest
import torch

from tests import pair_oracle_harness as H
from tests import pair_upstream_cases as PU

pytestmark = pytest.mark.gpu

SHAPES = ("W1", "I")


def _call(run, name, seed, path, up, poison=True, want=H.LEAVES):
    """one forward through ``path`` with the usual checks of flows and losses: (result, leaves)"""
    what = f"{name} {path} seed {seed}"
    mean_of = up.with_mean if up is not None else "sum"
    res, leaves = run.fused(seed, path, H.crit_code("l1"), poison=poison, with_mean=mean_of, want=want)
    assert res is not None, f"{what}: the fused path must take this case"
    H.check_values(name, what, res, H.oracle_forward(name, seed)["flows"], H.oracle(name, seed), "l1", sparse=True, mean_of=mean_of)
    return res, leaves


def _grads(run, res, leaves, up, **kw):
    lf, lb, _, lsum, mean = res
    return torch.autograd.grad(run.total(lf, lb, lsum, mean, up), leaves, **kw)


# ---------------------------------------------------------------------------------------------------
# a. subsets of the four outputs
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_mean", ["sum", "fwd"])
@pytest.mark.parametrize("subset", list(PU.SUBSETS))
@pytest.mark.parametrize("path", ["step", "node"])
@pytest.mark.parametrize("name", SHAPES)
def test_a_subset_of_the_outputs_in_the_loss(cuda, monkeypatch, name, path, subset, with_mean):
    """each output alone, three pairs, all four; the mean over loss_fwd + loss_bwd and over loss_fwd alone (``mean/fwd``: the
    oracle's gradient with a zero coefficient for loss_bwd -- frame 1's images contribute nothing).  ``bwd`` alone on the step
    path is the call ``launch_unit_scatter_tiles`` used to refuse."""
    up = PU.SPECS[f"{subset}/{with_mean}"](H.CASES[name]["B"])
    H.fused_case(cuda, monkeypatch, name, path, upstream=up, calls=1)


class _Drop(torch.autograd.Function):
    """identity whose backward hands on NO gradient: the node below is run with every incoming gradient undefined"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("path", ["step", "node"])
@pytest.mark.parametrize("name", SHAPES)
def test_no_output_in_the_loss(cuda, monkeypatch, name, path):
    """the flows alone are used (they carry no gradient: nothing to run backwards), and a backward in which no output
    receives a gradient: every leaf's gradient is None and no launch fails"""
    case = H.CASES[name]
    run = H.Run(cuda, monkeypatch, name)
    try:
        res, leaves = _call(run, name, case["seed"], path, None)
        lf, lb, flows, lsum, mean = res
        assert not flows[0].requires_grad and not flows[1].requires_grad
        assert run.total(lf, lb, lsum, mean, H.Upstream()) is None
        dummy = torch.zeros((), device=cuda, requires_grad=True)
        got = torch.autograd.grad(torch.nan_to_num(flows[0]).sum() + dummy, leaves + [dummy], allow_unused=True, retain_graph=True)
        assert all(g is None for g in got[:4]) and float(got[4]) == 1.0
        total = sum(_Drop.apply(x).sum() for x in (lf, lb, lsum, mean))
        got = torch.autograd.grad(total, leaves, allow_unused=True)
        assert all(g is None for g in got), [None if g is None else tuple(g.shape) for g in got]
        torch.cuda.synchronize(cuda)
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------
# b. magnitudes, signs, exact zeros
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,path,spec", [("W1", "step", "spread"), ("W1", "node", "spread"), ("I", "step", "spread"),
                                            ("W1", "step", "cancel"), ("W1", "node", "cancel")])
def test_magnitudes_signs_and_exact_zeros(cuda, monkeypatch, name, path, spec):
    """``spread``: coefficients 2^-100 .. 2^100 of both signs across the samples of one call, a sample whose coefficients are
    zero because its weights are; ``cancel``: a sample whose coefficients cancel exactly, every term non-zero.  The zero
    samples' gradients are exactly zero (no NaN), a sample with one zero coefficient gets the other direction's gradient
    alone, every other element stays within the rule at its own sample's magnitude."""
    B = H.CASES[name]["B"]
    up = PU.SPECS[spec](B)
    zero = tuple(b for b in PU.ZERO_GRAD_SAMPLES[spec] if b < B)
    assert zero
    H.fused_case(cuda, monkeypatch, name, path, upstream=up, grad_zero_samples=zero, calls=1)


def test_a_loss_scaler(cuda, monkeypatch):
    """every weight times 2^16: the gradients are the unscaled call's times 2^16 to within the rule, and the oracle's"""
    name, path = "W1", "step"
    case = H.CASES[name]
    up = PU.SPECS["all/sum"](case["B"])
    run = H.Run(cuda, monkeypatch, name)
    try:
        out = []
        for u in (up, up.scaled(PU.LOSS_SCALE)):
            res, leaves = _call(run, name, case["seed"], path, u)
            g = _grads(run, res, leaves, u)
            H.check_grads(name, f"{name} {path} scale {u.wf[0] / up.wf[0]:g}", g, H.oracle(name, case["seed"], upstream=u))
            out.append([x.double().cpu().numpy() for x in g])
        ref = H.oracle(name, case["seed"], upstream=up.scaled(PU.LOSS_SCALE))["grads"]
        worst = 0.0
        for a, b, r in zip(out[0], out[1], ref):
            tol = 1e-4 * np.abs(r) + 1e-5 * np.abs(r).max(axis=(1, 2), keepdims=True)
            worst = max(worst, H.units(np.abs(b - a * PU.LOSS_SCALE), tol))
        print(f"PAIR-UPSTREAM {name} {path}: scaled call against 2^16 x the unscaled call: {worst:.3f} of the rule")
        assert worst <= 1.0
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------
# c. the denormal end, d. non-finite upstream
# ---------------------------------------------------------------------------------------------------


def _one_odd_sample(cuda, monkeypatch, name, path, spec, b_odd, check_odd):
    """a spec one of whose samples has a coefficient outside the normal range: the others by the rule against the oracle of
    the spec with that sample's weights zeroed; the odd one by ``check_odd(leaf, got [V,3] float64, Gf, Gb)``"""
    case = H.CASES[name]
    B, seed = case["B"], case["seed"]
    up = PU.SPECS[spec](B)
    wf, wb = up.wf.copy(), up.wb.copy()
    wf[b_odd] = wb[b_odd] = 0
    rest = H.Upstream(wf, wb)
    run = H.Run(cuda, monkeypatch, name)
    try:
        res, leaves = _call(run, name, seed, path, up)
        grads = _grads(run, res, leaves, up)
        H.check_grads(name, f"{name} {path} {spec}", grads, H.oracle(name, seed, upstream=rest), samples=[b for b in range(B) if b != b_odd])
        Gf, Gb = H.oracle_units(name, seed)
        for g, f, b, leaf in zip(grads, Gf, Gb, H.LEAVES):
            check_odd(leaf, g[b_odd].double().cpu().numpy(), f[b_odd], b[b_odd])
    finally:
        run.close()


@pytest.mark.parametrize("path", ["step", "node"])
def test_the_denormal_end(cuda, monkeypatch, path):
    """sample 1's two coefficients are 2^-140: its gradients leave fp32's normal range.  Every element finite and within
    2^-126 of the oracle (flushing to zero passes, anything larger does not); the other samples within the rule."""
    kept = []

    def check(leaf, got, Gf, Gb):
        ref = 2.0 ** -140 * (Gf + Gb)
        assert np.isfinite(got).all(), leaf
        err = float(np.abs(got - ref).max())
        kept.append((int((got != 0).sum()), int((ref != 0).sum())))
        print(f"PAIR-UPSTREAM W1 {path} denormal: d/d {leaf}: largest |ref| {np.abs(ref).max():.3e}, largest error {err:.3e} "
              f"({err / 2.0 ** -126:.2e} of 2^-126), non-zero elements {kept[-1][0]} (oracle {kept[-1][1]})")
        assert err <= 2.0 ** -126, leaf

    _one_odd_sample(cuda, monkeypatch, "W1", path, "denormal", 1, check)
    # what reaches the node: torch's own backward of (loss x weight).sum() hands the weight on as it is, or flushed
    x = torch.ones(4, device=cuda, requires_grad=True)
    handed = torch.autograd.grad((x * torch.from_numpy(PU.SPECS["denormal"](4).wf).to(cuda)).sum(), x)[0]
    count = 3.0 * float(H.oracle("W1", H.CASES["W1"]["seed"])["full_masks"][0][1].sum())  # (of loss_fwd's direction)
    print(f"PAIR-UPSTREAM W1 {path} denormal: torch hands the node {float(handed[1]):.3e} (2^-140 = {2.0 ** -140:.3e}); the kernel's coefficient "
          f"is that over the sample's count ({count:.0f}): {2.0 ** -140 / count:.2e}, below fp32's smallest denormal {2.0 ** -149:.2e}; "
          f"the device {'KEPT denormals' if any(k for k, _ in kept) else 'returned the sample as zeros'}")


@pytest.mark.parametrize("path", ["step", "node"])
@pytest.mark.parametrize("spec,b_odd,direction", [("inf", 1, "fwd"), ("nan", 2, "bwd")])
def test_a_non_finite_upstream(cuda, monkeypatch, path, spec, b_odd, direction):
    """one sample's loss_fwd weight is +inf / another's loss_bwd weight is NaN: values, nothing faults.  Every gradient element
    of that sample that the oracle of that direction (weight 1) has non-zero is non-finite on the device (elements it has at
    exactly zero are not compared); every other sample stays within the rule.  The ``finite == false`` path: fp32 atomics."""
    def check(leaf, got, Gf, Gb):
        unit = Gf if direction == "fwd" else Gb
        live = unit != 0
        assert live.any(), leaf
        bad = int(np.isfinite(got[live]).sum())
        print(f"PAIR-UPSTREAM W1 {path} {spec}: d/d {leaf}: {int(live.sum())} elements the oracle has non-zero, {bad} of them finite on the device")
        assert bad == 0, leaf

    _one_odd_sample(cuda, monkeypatch, "W1", path, spec, b_odd, check)


# ---------------------------------------------------------------------------------------------------
# e. headroom
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", ["default", "spread"])
@pytest.mark.parametrize("name", list(PU.CASES))
def test_headroom(cuda, monkeypatch, name, spec):
    """wall scenes whose every workgroup sums with headroom 1 (X1) and 2 (X2) -- proven on the host from the oracle's coverage,
    which has to be the device's --, rule unchanged; the default weights through two calls of one plan, and the spread"""
    case = H.CASES[name]
    B, is_ = case["B"], case["raster"]
    up = None if spec == "default" else PU.SPECS[spec](B)
    worst = H.fused_case(cuda, monkeypatch, name, "step", upstream=up, calls=2 if up is None else 1)
    print(f"PAIR-UPSTREAM {name} {spec}: headroom {PU.HEADROOM[name]}, gradients {worst:.3f} of the rule")
    # the device's coverage is the oracle's: the host proof describes this run
    run = H.Run(cuda, monkeypatch, name)
    try:
        res, _ = run.fused(case["seed"], "step", H.crit_code("l1"))
        hit = res[2][0]._base._hoc_coverage[0]
        words = hit.contiguous().view(torch.int32).view(2 * B, -1) != 0
        assert words.sum(1).cpu().tolist() == PU.covered_tiles(H.oracle_forward(name, case["seed"]), is_)
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------
# f. which leaves want a gradient, g. two backwards through one forward
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("path", ["step", "node"])
def test_which_leaves_want_a_gradient(cuda, monkeypatch, path):
    """hand 1 alone, object 2 alone, both leaves of frame 2, all four: the wanted gradients are the oracle's (and so the
    all-four run's) within the rule, the others come back None, losses and flows are bit-identical across the runs"""
    name = "W1"
    case = H.CASES[name]
    up = PU.SPECS["all/sum"](case["B"])
    orc = H.oracle(name, case["seed"], upstream=up)
    run = H.Run(cuda, monkeypatch, name)
    try:
        outs = []
        for want in (H.LEAVES, ("hand 1",), ("object 2",), ("hand 2", "object 2")):
            res, leaves = _call(run, name, case["seed"], path, up, want=want)
            lf, lb, flows, lsum, mean = res
            run.total(lf, lb, lsum, mean, up).backward()
            assert [leaf.requires_grad for leaf in leaves] == [n in want for n in H.LEAVES]
            H.check_grads(name, f"{name} {path} wants {'+'.join(want)}", [leaf.grad for leaf in leaves], orc, leaves=want)
            outs.append([x.detach().clone() for x in (lf, lb, lsum, mean.reshape(1))] + [torch.nan_to_num(flows[0]._base.detach(), nan=-7.0)])
        for other in outs[1:]:
            for x, y, label in zip(other, outs[0], ("loss_fwd", "loss_bwd", "loss_bwd + loss_fwd", "batch mean", "flows")):
                assert torch.equal(x, y), label
    finally:
        run.close()


def test_two_backwards_through_one_forward(cuda, monkeypatch):
    """retain_graph: the second call clears the gradient buffer itself (GRAD_BUFFER_USED).  Other signs, other magnitudes and
    a zero sample in the second: each call against its own oracle, the zero sample exactly zero -- nothing of the first is left"""
    from handobjectconsist_amd.warping import pairstep

    name = "W1"
    case = H.CASES[name]
    first, second = PU.SPECS["all/sum"](case["B"]), PU.SPECS["second"](case["B"])
    run = H.Run(cuda, monkeypatch, name)
    try:
        res, leaves = _call(run, name, case["seed"], "step", first)
        plan = next(iter(pairstep._PLANS.values()))
        g1 = _grads(run, res, leaves, first, retain_graph=True)
        assert not plan.st_b.flags & pairstep.GRAD_BUFFER_USED
        g1 = [g.clone() for g in g1]
        g2 = _grads(run, res, leaves, second)
        assert plan.st_b.flags & pairstep.GRAD_BUFFER_USED
        H.check_grads(name, f"{name} step first backward", g1, H.oracle(name, case["seed"], upstream=first))
        H.check_grads(name, f"{name} step second backward", g2, H.oracle(name, case["seed"], upstream=second), zero_samples=PU.ZERO_GRAD_SAMPLES["second"])
    finally:
        run.close()
