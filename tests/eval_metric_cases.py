"""Shared by tests/test_eval_metrics_host.py and tests/test_gpu_eval_metrics.py (a helper module: nothing pytest collects):
seeded cases for mr_eval_feed, the evaluation of its formulas (include/meshraster_hip.h) in any numpy dtype -- float64 is the
expected value, float32 the emulation of the kernel's operation order -- and the per-element bound of an fp32 evaluation,
computed from the inputs alone.  Nothing is taken from a run.

The bound, with u = 2^-24 and "2 n u sum |terms|" for a sum of n rounded products (twice the standard bound, as in
tests/mano_adapt_cases.py):

    cofactor c = x y - z w                         E_c   = 2 . 2 u (|x y| + |z w|)
    det = (a0 c00 + a1 c10) + a2 c20               E_det = 2 . 6 u D,  D = |a0| C00 + |a1| C10 + |a2| C20 (C = |x y| + |z w|)
    i = c / det                                    E_i   = (E_c + |i| E_det) / (|det| - E_det) + 2 ulp(i)    (inf when E_det >= |det|)
    x' = (i0 x + i1 y) + i2                        E_p   = E_i0 |x| + E_i1 |y| + E_i2 + 2 . 3 u (|i0 x| + |i1 y| + |i2|)
    d = (p - cp) - (t - ct)                        E_d   = E_p + E_cp + E_t + E_ct + 2 u (|p - cp| + |t - ct| + |d|)
    dist = sqrt((d0^2 + d1^2) + d2^2)              E     = sum_r E_d_r + 2 . 3 u dist + 2 ulp(dist)
        (the norm moves by at most the norm of what its argument moves by; three roundings under the root, halved by it, and
        the root's own)
    per-sample sum of K distances                  sum_k E_k + 2 K u sum_k dist_k + 2 ulp(sum)
    MR_EVAL_POINTS                                 E_p + E_cp + 2 u |p - cp|

A sample whose affine is exactly singular has no finite expected value: its rows are expected non-finite.
"""
import functools

import numpy as np

U = 2.0 ** -24
PER_POINT, PER_SAMPLE_SUM, POINTS = 0, 1, 2

# (B, K) of the per-point cases: one point, the hand's 21 joints, the 8 corners, a wave and its neighbours, more than one
# workgroup's stride, the per-point limit
POINT_SHAPES = [(1, 1), (2, 21), (3, 8), (2, 63), (2, 64), (2, 65), (1, 257), (1, 4096)]
SUM_POINTS = [1, 64, 65, 1000, 10000]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def dataset_affines(rng, B):
    """the dataset's kind: rotation x scale 0.3 .. 3, translation up to a few hundred pixels"""
    ang, s = rng.uniform(-np.pi, np.pi, B), rng.uniform(0.3, 3.0, B)
    a = np.zeros((B, 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 1, 0], a[:, 1, 1] = s * np.cos(ang), -s * np.sin(ang), s * np.sin(ang), s * np.cos(ang)
    a[:, :2, 2] = rng.uniform(-300, 300, (B, 2))
    a[:, 2, 2] = 1.0
    return a.astype(np.float32)


class Case:
    def __init__(self, name, pred, target, affine=None, affine_target=False, center=-1, mode=PER_POINT, singular=()):
        self.name, self.pred, self.target, self.affine = name, pred, target, affine
        self.affine_target, self.center, self.mode, self.singular = affine_target, center, mode, tuple(singular)
        for a in (pred, target, affine):
            if a is not None:
                a.setflags(write=False)

    def __repr__(self):
        return self.name

    def rows(self, b0, b1):
        """the same case restricted to samples [b0, b1)"""
        return Case(f"{self.name}[{b0}:{b1}]", self.pred[b0:b1].copy(), self.target[b0:b1].copy(),
                    None if self.affine is None else self.affine[b0:b1].copy(), self.affine_target, self.center, self.mode,
                    [s - b0 for s in self.singular if b0 <= s < b1])


def _points(rng, B, K, dims):
    """(pred, target): pixels for dims 2 (predictions a few pixels off), metres for dims 3 (a few centimetres off)"""
    if dims == 2:
        target = rng.uniform(0, 480, (B, K, 2))
        pred = target + rng.standard_normal((B, K, 2)) * 12.0
    else:
        target = rng.uniform(-0.2, 0.2, (B, K, 3)) + np.array([0.0, 0.0, 0.6])
        pred = target + rng.standard_normal((B, K, 3)) * 0.03
    return pred.astype(np.float32), target.astype(np.float32)


@functools.lru_cache(maxsize=None)
def feed_cases():
    cases = []
    for B, K in POINT_SHAPES:
        rng = np.random.default_rng(100 * K + B)
        p2, t2 = _points(rng, B, K, 2)
        aff = dataset_affines(rng, B)
        cases.append(Case(f"B{B}-K{K}-2d", p2, t2))
        cases.append(Case(f"B{B}-K{K}-2d-affine", p2, t2, aff))
        cases.append(Case(f"B{B}-K{K}-2d-affine-target", p2, t2, aff, affine_target=True))
        p3, t3 = _points(rng, B, K, 3)
        for center in sorted({c for c in (-1, 0, 9, K - 1) if c < K}):
            cases.append(Case(f"B{B}-K{K}-3d-center{center}", p3, t3, center=center))
    for K in SUM_POINTS:
        rng = np.random.default_rng(7000 + K)
        p2, t2 = _points(rng, 2, K, 2)
        p3, t3 = _points(rng, 2, K, 3)
        cases.append(Case(f"sum-K{K}-2d-affine", p2, t2, dataset_affines(rng, 2), mode=PER_SAMPLE_SUM))
        cases.append(Case(f"sum-K{K}-3d", p3, t3, mode=PER_SAMPLE_SUM))
    rng = np.random.default_rng(4242)
    p2, t2 = _points(rng, 2, 21, 2)
    cases.append(Case("points-K21-affine", p2, t2, dataset_affines(rng, 2), mode=POINTS))
    p3, t3 = _points(rng, 2, 21, 3)
    cases.append(Case("points-K21-3d-center9", p3, t3, center=9, mode=POINTS))
    cases += [near_singular_case(), singular_case()]
    return cases


def near_singular_case():
    """sample 1's affine has rows that nearly depend on each other: |det| = 0.004 against D = 8"""
    rng = np.random.default_rng(99)
    pred, target = _points(rng, 3, 21, 2)
    aff = dataset_affines(rng, 3)
    aff[1] = np.array([[1.0, 2.0, 30.0], [2.0, 4.004, 50.0], [0.0, 0.0, 1.0]], np.float32)
    return Case("near-singular", pred, target, aff)


def singular_case():
    """sample 1's affine is exactly singular (its determinant is 0 in fp32 and in fp64)"""
    rng = np.random.default_rng(98)
    pred, target = _points(rng, 3, 21, 2)
    aff = dataset_affines(rng, 3)
    aff[1] = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]], np.float32)
    return Case("singular", pred, target, aff, singular=(1,))


def nan_case():
    """sample 1's centre joint has a NaN coordinate: every row of that sample is NaN, no other"""
    rng = np.random.default_rng(97)
    pred, target = _points(rng, 3, 21, 3)
    pred[1, 9, 0] = np.nan
    return Case("nan-prediction", pred, target, center=9, singular=(1,))


def by_name(name):
    return {c.name: c for c in feed_cases()}[name]


EIGHT_JOBS = ["B2-K21-2d-affine", "B2-K21-2d-affine-target", "B2-K21-3d-center9", "B2-K21-3d-center-1", "sum-K1000-2d-affine",
              "sum-K65-3d", "B2-K65-2d", "points-K21-affine"]  # (all B = 2)


def ordered_sum(dist, dt):
    """the kernel's order: thread t of 256 adds k = t, t + 256, ..., the 64 lanes of a wave meet in a butterfly (xor 32 .. 1),
    the four waves are added in order"""
    B, K = dist.shape
    n = -(-K // 256) * 256
    padded = np.zeros((B, n), dt)  # (x + 0 = x: the padding changes no partial)
    padded[:, :K] = dist
    part = np.zeros((B, 256), dt)
    for r in range(n // 256):
        part = (part + padded[:, r * 256:(r + 1) * 256]).astype(dt)
    v = part.reshape(B, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, np.arange(64) ^ off]).astype(dt)
    s = v[:, 0, 0]
    for w in (1, 2, 3):
        s = (s + v[:, w, 0]).astype(dt)
    return s


def forward(case, dt):
    """the header's formulas in dtype ``dt``, operation by operation -> dict of intermediates and ``out``"""
    f = {}
    pred, target = case.pred.astype(dt), case.target.astype(dt)
    B, K, dims = pred.shape
    with np.errstate(all="ignore"):
        if case.affine is not None:
            a = [case.affine.astype(dt).reshape(B, 9)[:, i] for i in range(9)]
            pairs = {"c00": (4, 8, 5, 7), "c01": (2, 7, 1, 8), "c02": (1, 5, 2, 4), "c10": (5, 6, 3, 8), "c11": (0, 8, 2, 6),
                     "c12": (2, 3, 0, 5), "c20": (3, 7, 4, 6)}
            c = {n: a[x] * a[y] - a[z] * a[w] for n, (x, y, z, w) in pairs.items()}
            f["C"] = {n: np.abs(a[x] * a[y]) + np.abs(a[z] * a[w]) for n, (x, y, z, w) in pairs.items()}
            det = (a[0] * c["c00"] + a[1] * c["c10"]) + a[2] * c["c20"]
            f["D"] = np.abs(a[0]) * f["C"]["c00"] + np.abs(a[1]) * f["C"]["c10"] + np.abs(a[2]) * f["C"]["c20"]
            f["det"] = det
            f["inv"] = np.stack([c[n] / det for n in ("c00", "c01", "c02", "c10", "c11", "c12")], 1)  # [B,6]
            f["inv_names"] = ("c00", "c01", "c02", "c10", "c11", "c12")

        def side(pts, recover):
            v = np.zeros((B, K, 3), dt)
            v[:, :, :dims] = pts
            if recover:
                i = f["inv"][:, None, :]
                x, y = v[:, :, 0].copy(), v[:, :, 1].copy()
                v[:, :, 0] = (i[:, :, 0] * x + i[:, :, 1] * y) + i[:, :, 2]
                v[:, :, 1] = (i[:, :, 3] * x + i[:, :, 4] * y) + i[:, :, 5]
            return v

        has = case.affine is not None
        p, t = side(pred, has and not case.affine_target), side(target, has and case.affine_target)
        cp = p[:, case.center:case.center + 1] if case.center >= 0 else np.zeros((B, 1, 3), dt)
        ct = t[:, case.center:case.center + 1] if case.center >= 0 else np.zeros((B, 1, 3), dt)
        pc, tc = p - cp, t - ct
        d = pc - tc
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        f.update(pc=pc, tc=tc, d=d, dist=dist)
        if case.mode == PER_POINT:
            f["out"] = dist
        elif case.mode == PER_SAMPLE_SUM:
            f["out"] = ordered_sum(dist, dt) if dt == np.float32 else dist.sum(1)
        else:
            f["out"] = pc[:, :, :dims]
    return f


def reference(case):
    """-> (fp64 value, bound) of the case's output; both hold inf / NaN in the rows of a singular sample"""
    f = forward(case, np.float64)
    pred, target = case.pred.astype(np.float64), case.target.astype(np.float64)
    B, K, dims = pred.shape
    with np.errstate(all="ignore"):
        e_inv = None
        if case.affine is not None:
            det, inv = f["det"], f["inv"]
            e_det = 2 * 6 * U * f["D"]
            e_c = np.stack([2 * 2 * U * f["C"][n] for n in f["inv_names"]], 1)
            room = np.abs(det) - e_det
            e_inv = np.where(room[:, None] > 0, (e_c + np.abs(inv) * e_det[:, None]) / room[:, None] + 2 * ulp32(inv), np.inf)

        def side_err(pts, recover):
            e = np.zeros((B, K, 3))
            if recover:
                x, y = np.abs(pts[:, :, 0]), np.abs(pts[:, :, 1])
                i, ei = np.abs(f["inv"][:, None, :]), e_inv[:, None, :]
                e[:, :, 0] = ei[:, :, 0] * x + ei[:, :, 1] * y + ei[:, :, 2] + 2 * 3 * U * (i[:, :, 0] * x + i[:, :, 1] * y + i[:, :, 2])
                e[:, :, 1] = ei[:, :, 3] * x + ei[:, :, 4] * y + ei[:, :, 5] + 2 * 3 * U * (i[:, :, 3] * x + i[:, :, 4] * y + i[:, :, 5])
            return e

        has = case.affine is not None
        e_p, e_t = side_err(pred, has and not case.affine_target), side_err(target, has and case.affine_target)
        zero = np.zeros((B, 1, 3))
        e_cp = e_p[:, case.center:case.center + 1] if case.center >= 0 else zero
        e_ct = e_t[:, case.center:case.center + 1] if case.center >= 0 else zero
        if case.mode == POINTS:
            return f["out"], (e_p + e_cp + 2 * U * np.abs(f["pc"]))[:, :, :dims]
        e_d = e_p + e_cp + e_t + e_ct + 2 * U * (np.abs(f["pc"]) + np.abs(f["tc"]) + np.abs(f["d"]))
        e_dist = e_d.sum(-1) + 2 * 3 * U * f["dist"] + 2 * ulp32(f["dist"])
        if case.mode == PER_POINT:
            return f["dist"], e_dist
        total = f["dist"].sum(1)
        return total, e_dist.sum(1) + 2 * K * U * total + 2 * ulp32(total)


def check(what, got, case, factor=1.0):
    """``got`` within the bound of the fp64 value element by element, outside the singular samples, whose rows must be
    non-finite; prints and returns the largest error / bound"""
    ref, bound = reference(case)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    keep = np.ones(ref.shape[0], bool)
    for s in case.singular:
        keep[s] = False
        assert not np.isfinite(got[s]).any(), f"{what}: sample {s} must be non-finite"
    got, ref, bound = got[keep], ref[keep], bound[keep]
    assert np.isfinite(ref).all() and np.isfinite(bound).all(), f"{what}: the case has no finite expectation"
    assert np.isfinite(got).all(), f"{what}: non-finite values outside the singular samples"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(factor * bound, 1e-300)).max()) if err.size else 0.0
    print(f"EVAL-METRICS {what}: max |err| {float(err.max()) if err.size else 0.0:.3e}, largest err / bound {ratio:.4f}")
    assert (err <= factor * bound).all(), f"{what}: {int((err > factor * bound).sum())} of {err.size} elements beyond the bound (largest ratio {ratio:.3f})"
    return ratio


# ---- the layer test's feeds: uneven batches that grow a log of capacity 8 twice (8 -> 16 -> 32 rows) -------------------------
LAYER_BATCHES = (5, 7, 3, 9)
LAYER_CAPACITY = 8
LAYER_RANGE = (0, 0.2, 20)


@functools.lru_cache(maxsize=None)
def layer_feeds():
    """[(pred, target)] 3-D joints, K = 21, no centre: what DeviceEvalUtil and the restated EvalUtil are both fed"""
    rng = np.random.default_rng(2024)
    return [_points(rng, B, 21, 3) for B in LAYER_BATCHES]


def layer_case(i):
    pred, target = layer_feeds()[i]
    return Case(f"layer-feed{i}", pred.copy(), target.copy())


def measure_logs():
    """[(name, log [rows, K] fp32)] for mr_eval_measures: seeded distances with duplicates, an all-equal column, 0.0 and
    denormals, values exactly on thresholds"""
    logs = []
    for rows in (1, 2, 3, 63, 64, 65, 1000, 4097):
        for K in (1, 21):
            rng = np.random.default_rng(31 * rows + K)
            log = np.abs(rng.standard_normal((rows, K))).astype(np.float32) * np.float32(0.08)
            log[:, 0] = np.round(log[:, 0] * 50) / 50          # duplicates: multiples of 0.02
            if K > 3:
                log[:, 1] = np.float32(0.05)                   # an all-equal column
                log[:, 2] = np.where(rng.random(rows) < 0.5, 0.0, 1e-41).astype(np.float32)  # zeros and denormals
                log[:, 3] = (rng.integers(0, 101, rows)).astype(np.float32)  # integers: 0 and 100 are thresholds of (0, 100, 100)
                # exactly on a threshold (the fp32 value the comparison uses) and its upper neighbour, for every range
                grid = np.concatenate([thresholds32(*r)[1] for r in MEASURE_RANGES])
                grid = np.concatenate([grid, np.nextafter(grid, np.float32(np.inf))])
                log[:, 4] = grid[rng.integers(0, len(grid), rows)]
            logs.append((f"rows{rows}-K{K}", log))
    return logs


MEASURE_RANGES = [(0, 0.2, 20), (0, 0.5, 20), (0, 100, 100)]


def thresholds32(lo, hi, steps):
    """(fp64 linspace, the fp32 thresholds rounded toward -inf): d <= t64 for an fp32 d exactly when d <= t32"""
    t = np.linspace(lo, hi, steps)
    t32 = t.astype(np.float32)
    above = t32.astype(np.float64) > t
    t32[above] = np.nextafter(t32[above], np.float32(-np.inf))
    return t, t32
