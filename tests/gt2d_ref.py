"""Shared by tests/test_gt2d_host.py and tests/test_gpu_gt2d.py (a helper module: nothing pytest collects): the float64 numpy
evaluation of the 2-D ground truth (include/meshraster_hip.h, mr_gt2d_batch; datasets/gt2d.py) and the per-element bound on a
float32 evaluation of it.  Nothing here imports the package's arithmetic: padding is index arithmetic (``arange(length) % n``).

Base pixels.  From float32 inputs -- the vertex v, the placement [A | b], the intrinsics K, the width W -- the formulas are

    p = A v + b  (BANK only; POINTS3D hands p over)     hom = K p     x = hom_0 / hom_2,  y = hom_1 / hom_2     x = W - x (mirrored)

and the yardstick evaluates them in float64 on those same float32 values.  A float32 evaluation rounds every operator once,
|d| <= u = 2^-24 (Higham, Accuracy and Stability, lemma 3.1: k roundings on a term cost it at most gamma_k = k u / (1 - k u)):

  * p_j: a product, two additions of the three products, + b_j: four roundings on the longest path, so the float32 p differs from
    the exact one by at most  e_j = gamma_4 (sum_i |A_ji| |v_i| + |b_j|)   (POINTS3D: e_j = 0, p is an input);
  * hom_r: a product and two additions on the longest path, applied to the float32 p:  |hom^_r - hom_r| <= E_r with
        E_r = gamma_3 sum_j |K_rj| (|p_j| + e_j)  +  sum_j |K_rj| e_j
    (the first term is the evaluation's own rounding, scaled by sum |K_rj| |p_j|; the second is the error p brought along);
  * the division: hom^_0 / hom^_2 - hom_0 / hom_2 = ((hom^_0 - hom_0) hom_2 - hom_0 (hom^_2 - hom_2)) / (hom^_2 hom_2), so with
    x* = hom_0 / hom_2 exact and |hom^_2| >= |hom_2| - E_2 > 0
        D = (E_0 + |x*| E_2) / (|hom_2| - E_2)          -- the errors propagate through 1 / |hom_z|
    and the quotient's own rounding adds u (|x*| + D):   Q = D + u (|x*| + D)  (+ 2^-149: a quotient that rounds to a subnormal);
  * the mirror, one subtraction:  Q' = Q + u (|W - x*| + Q).

Element by element, from the inputs alone; infinite where |hom_2| <= E_2 (no case goes there: every point lies at z >= 0.2).
A BLAS that fuses a multiply-add, or sums the three products in another order, takes no rounding more: the host path's numpy
lies under the same bound, and so do both of the reference's spellings of the projection (ho3dv2.py:500-503, and fhbhands.py:417-422,
which multiplies the points by 1000 first: one more rounding on p, gamma_1 |p_j|, cancelled by nothing -- its distance to the
bound is what tests/test_gt2d_host.py shows, on every case).

POINTS2D: the base pixel is the input or W minus it, one IEEE subtraction: bit for bit.

Transformed pixels.  t_r = M_r0 x + M_r1 y + M_r2 on the float32 base pixel, float32 M: the host evaluates it in float64 and
rounds once.  Against the EXACT value of that expression (long double, 64 bits of mantissa: the products of two float32 values are
exact in it and the sum of three is off by far less than a float32 half-ulp) rounded to float32, a float64 evaluation in any order
gives that float32 number or its neighbour: at most one ulp."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


def gamma(k):
    return k * U / (1.0 - k * U)


def cyc(a, length):
    return a[np.arange(length) % len(a)]


def bank_points(verts, pose):
    """(p [V,3] float64, e [V,3]): the exact placement of float32 vertices by a float32 [A | b], and the bound on a float32 p"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    pose = np.asarray(pose, np.float32).astype(np.float64)
    A, b = pose[:, :3], pose[:, 3]
    return v.dot(A.T) + b, gamma(4) * (np.abs(v).dot(np.abs(A).T) + np.abs(b))


def base_ref(p, e, camintr, flip, width):
    """(base [P,2] float64, bound [P,2]) of exact points ``p`` [P,3] whose float32 copies are off by at most ``e``"""
    K = np.asarray(camintr, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        hom = p.dot(K.T)
        E = gamma(3) * (np.abs(p) + e).dot(np.abs(K).T) + e.dot(np.abs(K).T)
        star = hom[:, :2] / hom[:, 2:]
        room = np.abs(hom[:, 2:]) - E[:, 2:]
        D = np.where(room > 0, (E[:, :2] + np.abs(star) * E[:, 2:]) / room, np.inf)
        Q = D + U * (np.abs(star) + D) + TINY
        if flip:
            star = star.copy()
            star[:, 0] = float(width) - star[:, 0]
            Q[:, 0] = Q[:, 0] + U * (np.abs(star[:, 0]) + Q[:, 0])
    return star, Q


def base_float32(p, camintr, flip, width):
    """the kernel's float32 chain, operator by operator in numpy float32 (same parentheses): where an element is not finite, this
    is numpy's inf / NaN pattern"""
    p, K = np.asarray(p, np.float32), np.asarray(camintr, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = [(K[r, 0] * p[:, 0] + K[r, 1] * p[:, 1]) + K[r, 2] * p[:, 2] for r in range(3)]
        x, y = h[0] / h[2], h[1] / h[2]
        if flip:
            x = np.float32(width) - x
    return np.stack([x, y], 1).astype(np.float32)


def trans_exact(base, affine):
    """the exact affine of float32 base pixels, rounded once to float32 (long double)"""
    b, M = np.asarray(base, np.float32).astype(np.longdouble), np.asarray(affine, np.float32).astype(np.longdouble).reshape(2, 3)
    with np.errstate(invalid="ignore"):
        return np.stack([M[r, 0] * b[:, 0] + M[r, 1] * b[:, 1] + M[r, 2] for r in range(2)], 1).astype(np.float32)


def trans_float64(base, affine):
    """the kernel's float64 chain (same parentheses): the class of a non-finite element"""
    b, M = np.asarray(base, np.float32).astype(np.float64), np.asarray(affine, np.float32).astype(np.float64).reshape(2, 3)
    with np.errstate(invalid="ignore"):
        return np.stack([(M[r, 0] * b[:, 0] + M[r, 1] * b[:, 1]) + M[r, 2] for r in range(2)], 1).astype(np.float32)


def within_one_ulp(got, want):
    """float32 arrays: equal, or neighbours"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


def step(case, models=None):
    """The whole step of a built case (tests/gt2d_cases.build): per group a dict {kind: (base float64 [g,P,2], bound [g,P,2],
    exact: the POINTS2D kind, compared bit for bit)}, padded cyclically to the group's longest model."""
    out, lo = [], 0
    for g in case["groups"]:
        d = {}
        for kind in ("objverts2d", "handverts2d", "joints2d"):
            per = []
            for i in range(lo, lo + g):
                flip, W = bool(case["flip"][i]), case["width"][i]
                if kind == "objverts2d" and case.get("model") is not None:
                    p, e = bank_points(models[case["model"][i]][0], case["pose"][i])
                elif kind == "handverts2d" and case.get("points3d") is not None:
                    p = np.asarray(case["points3d"][i], np.float32).astype(np.float64)
                    e = np.zeros_like(p)
                elif kind == "joints2d" and case.get("points2d") is not None:
                    b = np.asarray(case["points2d"][i], np.float32).copy()
                    if flip:
                        b[:, 0] = np.float32(W) - b[:, 0]
                    per.append((b, np.zeros(b.shape)))
                    continue
                else:
                    continue
                per.append(base_ref(p, e, case["camintr"][i], flip, W))
            if per:
                longest = max(len(b) for b, _ in per)
                d[kind] = (np.stack([cyc(b, longest) for b, _ in per]), np.stack([cyc(q, longest) for _, q in per]), kind == "joints2d")
        out.append(d)
        lo += g
    return out


def check_step(what, got, ref, affine, groups, skip=()):
    """``got``: per group a dict of float32 numpy arrays (gt2d.KEYS).  Base pixels element by element under the bound (POINTS2D:
    bit for bit), transformed pixels within one ulp of the exact affine of the base pixels GOT.  ``skip``: (group, kind, frame,
    point) of the elements that are not finite by construction, checked by their caller.  Prints the largest error / bound
    before it asserts; returns it."""
    assert len(got) == len(ref), what
    worst, lo = 0.0, 0
    for k, (g, r) in enumerate(zip(got, ref)):
        assert set(g) == {key + s for key in r for s in ("", "_trans")}, (what, k, sorted(g))
        for kind, (want, bound, exact) in r.items():
            base, trans = g[kind], g[kind + "_trans"]
            assert base.dtype == np.float32 and trans.dtype == np.float32 and base.shape == trans.shape == want.shape, (what, k, kind, base.shape, want.shape)
            mask = np.ones(base.shape, bool)
            for sk in skip:
                if sk[0] == k and sk[1] == kind:
                    mask[sk[2], sk[3]] = False
            assert np.isfinite(base[mask]).all() and np.isfinite(trans[mask]).all(), f"{what} dict {k}: {kind} has an element nobody wrote"
            if exact:
                assert np.array_equal(base.view(np.int32), want.astype(np.float32).view(np.int32)), f"{what} dict {k}: {kind} is no copy"
            else:
                with np.errstate(invalid="ignore"):
                    err = np.abs(base.astype(np.float64) - want)
                assert np.isfinite(bound[mask]).all() and (bound[mask] > 0).all()
                ratio = float((err[mask] / bound[mask]).max()) if mask.any() else 0.0
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{what} dict {k}: {kind} outside the bound, err/bound {ratio:.3f}"
            for i in range(base.shape[0]):
                ok = within_one_ulp(trans[i], trans_exact(base[i], affine[lo + i])) | ~mask[i]
                assert ok.all(), f"{what} dict {k}: {kind}_trans frame {i} more than one ulp from the exact affine at {np.argwhere(~ok)[:5].tolist()}"
        lo += groups[k]
    print(f"GT2D {what}: largest base error / bound {worst:.3f}")
    return worst
