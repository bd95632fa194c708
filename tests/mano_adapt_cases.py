"""Shared by tests/test_mano_adapt_host.py and tests/test_gpu_mano_adapt.py (a helper module: nothing pytest collects): the
fp64 numpy evaluation of the adaptor stage's formulas (include/meshraster_hip.h, mr_mano_adapt_*) and the per-element
error bound of an fp32 evaluation, computed from the inputs alone.

    j[b,k,:] = sum_i weight[k,i] verts[b,i,:]     c[b] = j[b,center] (0 for -1)
    joints_out = j - c, verts_out = verts - c
    S[b] = sum_k g_joints[b,k] + sum_i g_verts[b,i]  (center >= 0)      gt = g_joints, row center reduced by S
    grad_verts[b,i] = g_verts[b,i] + sum_k weight[k,i] gt[b,k]           grad_weight[k,i] = sum_b sum_r gt[b,k,r] verts[b,i,r]

Bound of an element: 2 n 2^-24 x (sum of the absolute values of the terms that make up the element) + 2 units in the last
place of the result (the final subtraction or addition).  n is the element's number of terms: V for a joint, and again for
the centre; J + 2 for a vertex gradient, plus V + J for S where center >= 0; 3 B for a weight-gradient element.  The factor
2 is the margin over the standard bound n u sum |terms| of a sum of n rounded products in any order.  Terms are expanded
down to products of inputs: S counts as its V + J addends, each times the weight it meets.  Against the reference-run
fixture, whose values carry fp32 rounding of their own, the bound is doubled.
"""
import functools
import os

import numpy as np

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (B, V, J, center): partial waves, one lane, more joints than waves, the limits of the LDS budget
SHAPES = [(1, 778, 21, 9), (3, 778, 21, 0), (3, 778, 21, 20), (2, 778, 21, -1), (2, 1, 1, 0), (2, 5, 3, 2), (2, 64, 21, 9), (2, 65, 21, 9),
          (2, 257, 2, 1), (2, 4096, 32, 31)]


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "adaptor_ref.npz")) as data:
        return {k: data[k] for k in data.files}


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """float32 (verts, weight, g_verts, g_joints) of a case, seeded by the shape.  V = 778 and J = 21: the reference's trained
    weights (centre 0: its centre-0 file, otherwise the centre-9 file) and posed hands in millimetres; elsewhere seeded weights
    of mixed sign."""
    B, V, J, center = shape
    rng = np.random.default_rng(1000 * V + 10 * J + B + (center + 1) * 7)
    if (V, J) == (778, 21):
        fx = fixture()
        weight = fx["adaptor_c0" if center == 0 else "adaptor_c9"]
        verts = (fx["verts_mm"][np.arange(B) % 3] + rng.standard_normal((B, V, 3)) * 2.0).astype(np.float32)
    else:
        weight = (rng.standard_normal((J, V)) / np.sqrt(V)).astype(np.float32)
        verts = (rng.standard_normal((B, V, 3)) * 50.0).astype(np.float32)
    g_verts = rng.standard_normal((B, V, 3)).astype(np.float32)
    g_joints = rng.standard_normal((B, J, 3)).astype(np.float32)
    for a in (verts, weight, g_verts, g_joints):
        a.setflags(write=False)
    return verts, weight, g_verts, g_joints


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def forward_reference(verts, weight, center):
    """-> {name: (fp64 value, bound)} for verts_out and joints_out"""
    v, w = np.asarray(verts, np.float64), np.asarray(weight, np.float64)
    V = v.shape[1]
    j = np.einsum("ki,bir->bkr", w, v)
    a = np.einsum("ki,bir->bkr", np.abs(w), np.abs(v))  # sum |terms| of a joint
    if center >= 0:
        c, ac = j[:, center:center + 1], a[:, center:center + 1]
    else:
        c, ac = np.zeros_like(j[:, :1]), np.zeros_like(a[:, :1])
    joints, vo = j - c, v - c
    return {"joints_out": (joints, 2 * V * U * (a + ac) + 2 * ulp32(joints)),
            "verts_out": (vo, 2 * V * U * ac + 2 * ulp32(vo))}


def backward_reference(verts, weight, center, g_verts, g_joints):
    """-> {name: (fp64 value, bound)} for grad_verts, gt and grad_weight; g_verts / g_joints may be None (zeros)"""
    v, w = np.asarray(verts, np.float64), np.asarray(weight, np.float64)
    B, V, _ = v.shape
    J = w.shape[0]
    gv = np.zeros((B, V, 3)) if g_verts is None else np.asarray(g_verts, np.float64)
    gj = np.zeros((B, J, 3)) if g_joints is None else np.asarray(g_joints, np.float64)
    gt, gt_abs = gj.copy(), np.abs(gj)
    n_verts = J + 2
    if center >= 0:
        S = gj.sum(1) + gv.sum(1)
        SA = np.abs(gj).sum(1) + np.abs(gv).sum(1)
        gt[:, center] -= S
        gt_abs[:, center] += SA  # the addends of S, in absolute value
        n_verts += V + J
    grad_verts = gv + np.einsum("ki,bkr->bir", w, gt)
    t_verts = np.abs(gv) + np.einsum("ki,bkr->bir", np.abs(w), gt_abs)
    grad_weight = np.einsum("bkr,bir->ki", gt, v)
    t_weight = np.einsum("bkr,bir->ki", gt_abs, np.abs(v))
    return {"grad_verts": (grad_verts, 2 * n_verts * U * t_verts + 2 * ulp32(grad_verts)),
            "gt": (gt, 2 * (V + J) * U * gt_abs + 2 * ulp32(gt)),
            "grad_weight": (grad_weight, 2 * 3 * B * U * t_weight + 2 * ulp32(grad_weight))}


def check(what, got, ref_and_bound, factor=1.0):
    """``got`` within ``factor`` x the bound of the fp64 value, element by element; prints the largest error / bound ratio"""
    ref, bound = ref_and_bound
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    ratio = float((err / np.maximum(factor * bound, 1e-300)).max()) if err.size else 0.0
    print(f"MANO-ADAPT {what}: max |err| {float(err.max()) if err.size else 0.0:.3e}, largest err / bound {ratio:.4f}")
    assert (err <= factor * bound).all(), f"{what}: {int((err > factor * bound).sum())} of {err.size} elements beyond the bound (largest ratio {ratio:.3f})"
    return ratio
