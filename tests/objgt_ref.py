"""Shared by tests/test_objgt_host.py and tests/test_gpu_objgt.py (a helper module: nothing pytest collects): the float64 numpy
evaluation of the object ground truth (include/meshraster_hip.h, mr_obj_gt_batch; datasets/objgt.py), the per-element bound on a
float32 evaluation of it, and the cases both files use.  Nothing here imports the package's arithmetic: padding is index
arithmetic (``arange(length) % n``), not ``collate.pad_cyclic``; the canonical copy is plain numpy float32.

The bound.  objverts3d = R (A v + b) - c is evaluated in float32 from float32 inputs, except that the placement [A | b] may be
handed over in float64 and is then rounded to float32 once (the fold).  Roundings on the longest path from an input to an
output element, counted from csrc/obj_gt.hip and objgt.obj_geometry_host (the same chain; a BLAS that fuses a multiply-add
only takes roundings away):

    1  [A | b] float64 -> float32                    (pack_obj_info / frame_records: the fold's one rounding)
    1  A_ij * v_j
    2  the two additions of the three products
    1  + b_i
    1  R_ri * y_i                                    (R is a float32 input -- the mirror only flips signs: no rounding)
    2  the two additions of the three products
    1  - c_r
    -
    9  = K_ROUNDINGS

Each rounding multiplies what it is applied to by (1 + d), |d| <= u = 2^-24, so every term of the expanded sum carries at most
(1 + u)^9 - 1 <= gamma_9 = 9 u / (1 - 9 u) of relative error (Higham, Accuracy and Stability, lemma 3.1):

    |err_r| <= gamma_9 * ( sum_j (|R| |A|)_rj |v_j|  +  (|R| |b|)_r  +  |c_r| )

element by element, from the inputs alone."""
import numpy as np

U = 2.0 ** -24
K_ROUNDINGS = 9


def gamma(k):
    return k * U / (1.0 - k * U)


def canonical(verts):
    """numpy float32: box [6], centre [3], canverts [V,3] -- center_vert_bbox(verts, scale=False) as published"""
    v = np.asarray(verts, np.float32)
    lo, hi = v.min(0), v.max(0)
    centre = (lo + hi) * np.float32(0.5)
    return np.concatenate([lo, hi]), centre, v - centre


def frame(verts, pose, flip, rot_mat, center3d):
    """(objverts3d [V,3] float64, bound [V,3]) of one frame, unpadded.  ``pose`` as it was handed over (float64 or float32);
    ``rot_mat`` / ``center3d`` float32 or None."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    A, b = np.asarray(pose, np.float64)[:, :3], np.asarray(pose, np.float64)[:, 3]
    R = np.eye(3) if rot_mat is None else np.asarray(rot_mat, np.float32).astype(np.float64)
    c = np.zeros(3) if center3d is None else np.asarray(center3d, np.float32).astype(np.float64)
    y = v.dot(A.T) + b
    if flip:
        y[:, 0] = -y[:, 0]
    out = y.dot(R.T) - c
    mag = np.abs(v).dot((np.abs(R).dot(np.abs(A))).T) + np.abs(R).dot(np.abs(b)) + np.abs(c)
    return out, gamma(K_ROUNDINGS) * mag


def cyc(a, length):
    return a[np.arange(length) % len(a)]


def step(models, model, pose, flip, rot_mat, center3d, groups):
    """The whole step: per group a dict with objverts3d (float64) and its bound, and the bit-exact arrays objcanverts
    (float32), objfaces (int64), objcantrans, objcanscale -- padded cyclically to the group's longest model."""
    out, lo = [], 0
    for g in groups:
        idx = range(lo, lo + g)
        lo += g
        vmax = max((len(models[model[i]][0]) for i in idx), default=0)
        fmax = max((len(models[model[i]][1]) for i in idx), default=0)
        d = {k: [] for k in ("objverts3d", "bound", "objcanverts", "objfaces", "objcantrans")}
        for i in idx:
            verts, faces = models[model[i]]
            ref, bound = frame(verts, pose[i], bool(flip[i]) if flip is not None else False, None if rot_mat is None else rot_mat[i],
                               None if center3d is None else center3d[i])
            _, centre, can = canonical(verts)
            can = can.copy()
            if flip is not None and flip[i]:
                can[:, 0] = -can[:, 0]
            d["objverts3d"].append(cyc(ref, vmax))
            d["bound"].append(cyc(bound, vmax))
            d["objcanverts"].append(cyc(can, vmax))
            d["objfaces"].append(cyc(np.asarray(faces, np.int64), fmax))
            d["objcantrans"].append(centre)
        res = {k: np.stack(v) if g else np.zeros((0, 0, 3)) for k, v in d.items()}
        res["objcanscale"] = np.ones(g, np.float32)
        out.append(res)
    return out


def check_step(what, got, ref):
    """``got``: per group a dict of numpy arrays (objgt.KEYS).  objverts3d element by element under the bound, everything else
    bit for bit.  Prints the largest error / bound before it asserts."""
    assert len(got) == len(ref), what
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        n = r["objcanscale"].shape[0]
        if n == 0:
            assert all(len(g[key]) == 0 for key in ("objverts3d", "objcanverts", "objfaces", "objcantrans", "objcanscale")), (what, k)
            continue
        assert g["objverts3d"].dtype == np.float32 and g["objverts3d"].shape == r["objverts3d"].shape, (what, k, g["objverts3d"].shape)
        assert np.isfinite(g["objverts3d"]).all(), f"{what} dict {k}: objverts3d has an element nobody wrote"
        err = np.abs(g["objverts3d"].astype(np.float64) - r["objverts3d"])
        assert (r["bound"] > 0).all()
        worst = max(worst, float((err / r["bound"]).max()))
        bad = np.argwhere(err > r["bound"])
        assert not len(bad), f"{what} dict {k}: objverts3d outside the bound at {bad[:5].tolist()}, err/bound {float((err / r['bound']).max()):.3f}"
        for key, dt in (("objcanverts", np.float32), ("objcantrans", np.float32), ("objcanscale", np.float32), ("objfaces", np.int64)):
            assert g[key].dtype == dt and g[key].shape == r[key].shape, (what, k, key, g[key].dtype, g[key].shape)
            assert np.array_equal(g[key].view(np.int32 if dt == np.float32 else np.int64), np.ascontiguousarray(r[key], dtype=dt).view(
                np.int32 if dt == np.float32 else np.int64)), f"{what} dict {k}: {key} differs"
    print(f"OBJGT {what}: largest objverts3d error / bound {worst:.3f}")
    return worst


# ---- cases ------------------------------------------------------------------------------------------------------------------
BANK_V = (1, 2, 63, 64, 65, 257, 1031)   # a lane, a pair, one short of a wave, a wave, one over, a workgroup + 1, four strides + 7
BANK_F = (1, 2, 127, 128, 129, 128, 2)


def bank_models(seed=0):
    """seven models with BANK_V vertices and BANK_F faces: vertices a few centimetres around an offset origin, one axis of
    model 2 all equal (a flat box), random model-local faces"""
    rng = np.random.default_rng([seed, 7])
    models = []
    for k, (nv, nf) in enumerate(zip(BANK_V, BANK_F)):
        v = (rng.standard_normal((nv, 3)) * 0.05 + rng.standard_normal(3) * 0.02).astype(np.float32)
        if k == 2:
            v[:, 1] = np.float32(0.0125)
        models.append((v, rng.integers(0, nv, (nf, 3)).astype(np.int32)))
    return models


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).astype(np.float32)


def rotation(w):
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K.dot(K)


def step_args(model, flip, rot, center, scale, seed=0):
    """the frames ``model`` with every frame mirrored or none (``flip`` None: alternating), an augmentation rotation or the
    identity, a centre or none, and a placement A = scale * rotation (1: metres; 1 / 1000: a model stored in millimetres)"""
    rng = np.random.default_rng([seed, 11, len(model)])
    n = len(model)
    pose = np.stack([np.concatenate([scale * rotation(rng.standard_normal(3)), (rng.standard_normal((3, 1)) * 0.1 + [[0], [0], [0.6]])], 1)
                     for _ in range(n)]) if n else np.zeros((0, 3, 4))
    flips = np.arange(n) % 2 == 1 if flip is None else np.full(n, bool(flip))
    rot_mat = np.stack([rot_z(a) for a in rng.uniform(-np.pi, np.pi, n)]) if rot and n else (np.zeros((0, 3, 3), np.float32) if rot else None)
    center3d = (rng.standard_normal((n, 3)) * 0.1 + [0, 0, 0.6]).astype(np.float32) if center else None
    return dict(model=np.asarray(model, np.int64), pose=pose, flip=flips, rot_mat=rot_mat, center3d=center3d)


# five frames in two dicts whose maxima differ: the one-vertex / one-face model 0 padded to 65 rows (faces: 129) in the first
# dict and to 257 (faces: 128) in the second
FIVE = dict(model=[0, 4, 0, 5, 0], groups=[3, 2])
