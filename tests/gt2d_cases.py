"""The cases of the 2-D ground truth, shared by tests/test_gt2d_host.py and tests/test_gpu_gt2d.py (a helper module: nothing
pytest collects).  ``build(name)`` -> the arguments of ``gt2d.points2d_host`` / ``points2d_batch`` as float32 / integer numpy arrays
(what both the package and tests/gt2d_ref.py start from), plus ``skip``: the elements that are not finite by construction.

Models of 1, 20, 63, 64, 65 and 986 vertices (a lane, a small mesh, one short of a wave, a wave, one over, nearly four
workgroups) and one of 40 (twice the 20).  Every point lies at z >= 0.2 (``build`` asserts it): no case leans on the conditioning
near the camera plane -- except the one point of ``points3d-hom-z-zero``."""
import numpy as np

MODEL_V = (1, 20, 63, 64, 65, 986, 40)
WIDTHS = (640, 272)

# name -> what is in the step.  ``model``: the bank's model of each frame (BANK records), ``p3``: points a frame of POINTS3D
# records, ``p2``: of POINTS2D records, ``groups``: frames per collated dict, ``flip``: per frame.
CASES = {
    # padded to V itself: one frame, 986 rows (not a multiple of 256)
    "bank-one-frame": dict(model=[5], groups=[1], flip=[1]),
    # V + 1: the 64-vertex model beside the 65-vertex one; flips mixed inside the group
    "bank-v-plus-one": dict(model=[4, 3], groups=[2], flip=[0, 1]),
    # exact multiples: the 20-vertex model beside the 40-vertex one, and the single vertex (20 x 1, 40 x 1)
    "bank-exact-multiple": dict(model=[1, 6, 0], groups=[3], flip=[1, 0, 1]),
    # much larger: the 1-vertex model beside the 986-vertex one
    "bank-one-vertex-beside-986": dict(model=[0, 5], groups=[2], flip=[0, 1]),
    # seven frames in two dicts, every model once: two padded lengths in one launch
    "bank-seven-frames": dict(model=[0, 5, 2, 1, 6, 3, 4], groups=[3, 4], flip=[0, 1, 1, 1, 0, 0, 1]),
    # a step of exactly one row
    "bank-single-row": dict(model=[0], groups=[1], flip=[1]),
    "points3d-1": dict(p3=1, groups=[2], flip=[1, 0]),
    "points3d-65": dict(p3=65, groups=[2], flip=[0, 1]),
    "points3d-778": dict(p3=778, groups=[1, 1], flip=[1, 0]),
    "points2d-21": dict(p2=21, groups=[2, 1], flip=[0, 1, 1]),
    # three dicts, all three kinds: what a training step asks for
    "mixed-three-dicts": dict(model=[5, 0, 2, 6, 1], p3=778, p2=21, groups=[2, 1, 2], flip=[0, 1, 1, 0, 1]),
    # one point on the camera plane: hom_z == 0, inf / NaN in its own two elements
    "points3d-hom-z-zero": dict(p3=65, groups=[2], flip=[0, 1], zero=(1, 17)),
}


def models(seed=0):
    """the seven models: vertices a few centimetres around the origin, random model-local faces"""
    rng = np.random.default_rng([seed, 23])
    return [((rng.standard_normal((nv, 3)) * 0.04).astype(np.float32), rng.integers(0, nv, (max(nv // 2, 1), 3)).astype(np.int32)) for nv in MODEL_V]


def rotation(w):
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K.dot(K)


def crop_affine(center, scale, res, rot):
    """rows 0 and 1 of the crop affine (rotation about the origin, then the crop around the rotated centre), float32"""
    c, s = np.cos(rot), np.sin(rot)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    centre = R.dot([center[0], center[1], 1.0])
    crop = np.array([[res / scale, 0.0, res * (0.5 - centre[0] / scale)], [0.0, res / scale, res * (0.5 - centre[1] / scale)], [0.0, 0.0, 1.0]])
    return crop.dot(R)[:2].astype(np.float32)


def build(name, seed=0):
    spec = CASES[name]
    n = sum(spec["groups"])
    rng = np.random.default_rng([seed, 29, sorted(CASES).index(name)])
    width = np.array([WIDTHS[i % 2] for i in range(n)], np.float32)  # two widths in one launch
    camintr = np.zeros((n, 3, 3), np.float32)
    for i in range(n):  # a different K per frame
        camintr[i] = [[rng.uniform(450, 620), rng.uniform(-0.5, 0.5), width[i] / 2 + rng.uniform(-8, 8)], [0, rng.uniform(450, 620), 0.375 * width[i] + rng.uniform(-8, 8)],
                      [0, 0, 1]]
    affine = np.stack([crop_affine((width[i] / 2 + rng.uniform(-40, 40), 0.375 * width[i] + rng.uniform(-40, 40)), rng.uniform(120, 260), 256,
                                   rng.uniform(-np.pi, np.pi)) for i in range(n)])
    case = dict(camintr=camintr, flip=np.asarray(spec["flip"], bool), width=width, affine=affine, groups=list(spec["groups"]), skip=[])
    centre = lambda: rng.standard_normal(3) * [0.08, 0.06, 0.1] + [0, 0, 0.6]
    if "model" in spec:
        case["model"] = np.asarray(spec["model"], np.int64)
        case["pose"] = np.stack([np.concatenate([rotation(rng.standard_normal(3)), centre()[:, None]], 1) for _ in range(n)]).astype(np.float32)
        mods = models()
        for i in range(n):
            v = mods[case["model"][i]][0].astype(np.float64)
            assert (v.dot(case["pose"][i][:, :3].astype(np.float64).T) + case["pose"][i][:, 3])[:, 2].min() >= 0.2
    if "p3" in spec:
        case["points3d"] = np.stack([rng.standard_normal((spec["p3"], 3)) * 0.04 + centre() for _ in range(n)]).astype(np.float32)
        assert case["points3d"][..., 2].min() >= 0.2
        if "zero" in spec:
            frame, point = spec["zero"]
            case["points3d"][frame, point] = [0.1, -0.2, 0.0]
            group = int(np.searchsorted(np.cumsum(spec["groups"]), frame, side="right"))
            case["skip"].append((group, "handverts2d", frame - sum(spec["groups"][:group]), point))
    if "p2" in spec:
        case["points2d"] = (rng.uniform(0, 1, (n, spec["p2"], 2)) * np.stack([width, 0.75 * width], 1)[:, None]).astype(np.float32)
    return case


def call_args(case):
    """the keyword arguments of ``gt2d.points2d_host`` / ``points2d_batch`` (less the bank)"""
    return {k: v for k, v in case.items() if k != "skip"}
