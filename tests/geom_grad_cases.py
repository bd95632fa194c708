"""Inputs, references and the tolerance rule shared by tests/test_geom_grad_ref_host.py (CPU: the references and the
conditions on them) and tests/test_gpu_mano_grads.py / tests/test_gpu_post_grads.py (the kernels).  A helper module: no
fixtures, nothing pytest collects.

The rule: a kernel's error against the float64 reference, per tensor and normalised per sample
(``geom_grad_ref.per_sample_error``), may be at most ``FACTOR`` times the error ``e_y`` of the YARDSTICK in the same case and
tensor -- the same formulas evaluated in fp32 on the CPU with torch autograd (``SynthManoLayer.forward_torch``;
``geom_grad_ref.post_forward`` on float32 tensors).  The conditions below keep the rule from going slack; the host file
checks them for every input a GPU case uses, so a seed whose yardstick breaks one is an error of this file."""
import contextlib
import functools

import numpy as np
import torch

from oracle import geom_grad_ref as R
from oracle import mano_ref as M

FACTOR = 4.0             # kernel error <= FACTOR * e_y (wave shuffles, split-K partials and float atomics against pairwise sums)
MAX_DISAGREEMENT = 1e-7  # central differences at eps against 10 eps, per sample and component
MAX_EY_GRAD = 2.5e-6     # the yardstick's own error, gradients
MAX_EY_VALUE = 1e-6      # ... and values: no case ever accepts more than FACTOR * these
EPS = 1e-6


@contextlib.contextmanager
def one_cpu_thread():
    """The yardstick runs on ONE thread: MKL splits its fp32 reductions by the thread count, and the same case read
    1.2e-6 on eight threads and 2.6e-6 on four (grad betas, tip centre 8).  A yardstick has to be the same number in the host
    file and in the GPU run, whatever ran before it in the process."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(before)


class Report:
    """One case's comparisons: ``add`` measures a tensor of the kernel and of the yardstick against the reference, ``finish``
    prints ONE line with every figure and only then asserts -- the figures of a failing case are in the output too.
    ``limit`` is the condition the host file holds the yardstick to: a yardstick that is worse than that on the machine of
    the GPU run (the fp32 BLAS and libm of another CPU) buys the kernel nothing, the bound stops at ``factor * limit``."""

    def __init__(self, case):
        self.case, self.items, self.failures = case, [], []

    def add(self, what, got, yard, ref, limit, factor=FACTOR):
        e_y, e_k = R.per_sample_error(yard, ref), R.per_sample_error(got, ref)
        self.items.append(f"{what} {e_y:.2e}/{e_k:.2e}")
        if not e_k <= factor * min(e_y, limit):
            self.failures.append(f"{what}: kernel error {e_k:.3e} > {factor:g} x yardstick {min(e_y, limit):.3e}")
        return e_y, e_k

    def finish(self):
        print(f"{self.case}: yardstick/kernel " + " ".join(self.items))
        assert not self.failures, f"{self.case}: " + "; ".join(self.failures)


# ------------------------------------------------------------------------------------------------ MANO
BUFFERS = ("th_v_template", "th_shapedirs", "th_posedirs", "th_J_regressor", "th_weights", "th_comps", "th_hands_mean")
B_MASTER = 33
# entry point, use_pca, flat_hand_mean, center_idx, translation ("none" | "given" | "zeros").  The six of
# test_gpu_mano_full.VARIANTS through forward_full, then ``forward`` where it applies, then manopth's all-zero rule
MANO_VARIANTS = {
    "full-axisang-flat-uncentred": ("forward_full", False, True, None, "none"),
    "full-axisang-centre9": ("forward_full", False, False, 9, "none"),
    "full-pca-tip4": ("forward_full", True, False, 4, "none"),
    "full-pca-tip8": ("forward_full", True, False, 8, "none"),
    "full-pca-tip20": ("forward_full", True, False, 20, "none"),
    "full-pca-centre9-trans": ("forward_full", True, False, 9, "given"),
    "forward-pca-centre9": ("forward", True, False, 9, "none"),
    "forward-pca-uncentred": ("forward", True, False, None, "none"),
    "full-pca-centre9-zero-trans": ("forward_full", True, False, 9, "zeros"),
}
# samples of the master batch a run takes: B = 1 twice (the zero root rotation; the one near pi), one full batch tile of 32,
# one sample in a second tile
MANO_RUNS = {"B1-zero-root": [0], "B1-root-3.1": [2], "B32": list(range(32)), "B33": list(range(33))}
TIP_ROWS = [k for k, src in enumerate(M.REORDER) if src >= 16]  # output rows 4, 8, 12, 16, 20: skinned vertices, not the chain
MANO_WEIGHTS = ("dense", "verts-only", "joints-only", "vertex-777-and-0", "tips-only", "zero")


def make_layer(variant):
    from handobjectconsist_amd.models import synthnet

    _, use_pca, flat, center_idx, _ = MANO_VARIANTS[variant]
    return synthnet.SynthManoLayer(ncomps=15, use_pca=use_pca, flat_hand_mean=flat, center_idx=center_idx)


def layer_consts(layer):
    return {k: getattr(layer, k).detach().cpu().numpy().astype(np.float64) for k in BUFFERS}


def mano_inputs(variant):
    """(pose, betas, trans | None) of the master batch, fp32 tensors.  Keyed on the layer, not on the translation: the
    all-zero-translation variant shares the inputs (and the reference) of ``forward-pca-centre9``."""
    _, use_pca, flat, center_idx, trans_kind = MANO_VARIANTS[variant]
    g = torch.Generator().manual_seed(4100 + 100 * use_pca + 10 * flat + (center_idx if center_idx is not None else 30))
    pose = 0.4 * torch.randn(B_MASTER, 18 if use_pca else 48, generator=g)
    pose[0, :3] = 0                                          # the 1e-8 guard of the Rodrigues formula
    pose[1, :3] = torch.tensor([1e-6, 0.0, 0.0])
    pose[2, :3] = 3.1 * torch.tensor([0.6, -0.64, 0.48])     # a root rotation of 3.1 rad, close to pi
    betas = torch.randn(B_MASTER, 10, generator=g)
    trans = None
    if trans_kind == "given":
        trans = 0.1 * torch.randn(B_MASTER, 3, generator=g)
        trans[3] = 0                                         # zero for ONE sample only: still in force for every sample
    elif trans_kind == "zeros":
        trans = torch.zeros(B_MASTER, 3)
    return pose, betas, trans


def mano_weights(pattern):
    """(w_verts [33,778,3] | None, w_joints [33,21,3] | None): None = that output does not enter the loss at all (the
    backward entry point then gets a null pointer)."""
    g = torch.Generator().manual_seed(977)
    wv, wj = torch.randn(B_MASTER, 778, 3, generator=g), torch.randn(B_MASTER, 21, 3, generator=g)
    if pattern == "dense":
        return wv, wj
    if pattern == "verts-only":
        return wv, None
    if pattern == "joints-only":
        return None, wj
    if pattern == "vertex-777-and-0":  # 777: the last of the 10 vertices in the fourth 256-thread chunk of the skin adjoint
        keep = torch.zeros(778, 1)
        keep[[0, 777]] = 1
        return wv * keep, None
    if pattern == "tips-only":
        keep = torch.zeros(21, 1)
        keep[TIP_ROWS] = 1
        return None, wj * keep
    if pattern == "zero":
        return torch.zeros_like(wv), torch.zeros_like(wj)
    raise KeyError(pattern)


def _dense(w, shape):
    return np.zeros(shape) if w is None else w.double().numpy()


# an all-zero translation is an absent one: the same layer, the same inputs, the same reference
_SAME_REFERENCE = {"full-pca-centre9-zero-trans": "forward-pca-centre9"}


def mano_reference(variant, eps=EPS):
    """float64 values and the Jacobian of the master batch: the expensive part, once per layer whatever the weights"""
    return _mano_reference(_SAME_REFERENCE.get(variant, variant), eps)


@functools.lru_cache(maxsize=2)
def _mano_reference(variant, eps):
    _, use_pca, _, center_idx, _ = MANO_VARIANTS[variant]
    c = layer_consts(make_layer(variant))
    pose, betas, trans = mano_inputs(variant)
    kw = dict(use_pca=use_pca, center_idx=center_idx)
    t = None if trans is None else trans.double().numpy()
    verts, joints = M.mano_forward(c, pose.double().numpy(), betas.double().numpy(), trans=t, **kw)
    jac = R.mano_jacobian(c, pose.double().numpy(), betas.double().numpy(), t, eps=eps, **kw)
    return verts, joints, jac


def mano_reference_gradients(variant, pattern, eps=EPS):
    """{"pose", "betas", "trans"} of the master batch in float64 (an absent translation: zeros, what its gradient has to be)"""
    _, _, jac = mano_reference(variant, eps)
    wv, wj = mano_weights(pattern)
    grads = R.mano_gradients(None, None, None, None, _dense(wv, (B_MASTER, 778, 3)), _dense(wj, (B_MASTER, 21, 3)),
                             jacobian=jac)
    if grads["trans"] is None and MANO_VARIANTS[variant][4] != "none":
        grads["trans"] = np.zeros((B_MASTER, 3))
    return grads


def mano_run(layer, entry, pose, betas, trans, wv, wj):
    """one forward + backward of ``layer`` through ``entry`` ("forward" | "forward_full"): the kernels on a GPU, the fp32 torch
    restatement on the CPU -> values and gradients, tensors on the layer's device; ``wv`` / ``wj`` None = output unused"""
    dev = layer.th_v_template.device
    with one_cpu_thread() if dev.type == "cpu" else contextlib.nullcontext():
        return _mano_run(layer, entry, dev, pose, betas, trans, wv, wj)


def _mano_run(layer, entry, dev, pose, betas, trans, wv, wj):
    p, b_ = pose.to(dev).requires_grad_(True), betas.to(dev).requires_grad_(True)
    t_ = None if trans is None else trans.to(dev).requires_grad_(True)
    verts, joints = layer.forward_full(p, b_, t_) if entry == "forward_full" else layer(p, b_)
    loss = sum((o * w.to(dev)).sum() for o, w in ((verts, wv), (joints, wj)) if w is not None)
    loss.backward()
    out = {"verts": verts.detach(), "joints": joints.detach(), "pose": p.grad, "betas": b_.grad}
    if t_ is not None:
        out["trans"] = t_.grad if t_.grad is not None else torch.zeros_like(t_)
    return out


def as_f64(tensors):
    return {k: v.double().cpu().numpy() for k, v in tensors.items()}


def mano_case_inputs(variant, run, pattern):
    """the fp32 inputs of one run: (pose, betas, trans | None, wv | None, wj | None)"""
    rows = MANO_RUNS[run]
    return tuple(None if a is None else a[rows] for a in mano_inputs(variant) + mano_weights(pattern))


def mano_case(variant, run, pattern):
    """... and its float64 reference: values and gradients of the same rows"""
    verts, joints, _ = mano_reference(variant)
    ref = dict(mano_reference_gradients(variant, pattern), verts=verts, joints=joints)
    return mano_case_inputs(variant, run, pattern) + ({k: None if v is None else v[MANO_RUNS[run]] for k, v in ref.items()},)


# ------------------------------------------------------------------------------------------------ head post-processing
POST_CONSTS = (100.0, 0.0001, 0.4, (256.0, 240.0))  # trans_factor, scale_factor, off_z, (res_w, res_h): the trainer's
# (B, Vh, J, Vo): each block covers 256 points, the grid is ceil(max(Vh + J, Vo) / 256), hand and object share a thread index
POST_SHAPES = [(1, 778, 21, 1), (6, 778, 21, 1002), (6, 250, 6, 256), (6, 250, 6, 257), (2, 255, 2, 3), (2, 5, 3, 0),
               (2, 0, 0, 40)]
POST_OUTPUTS = ("handverts3d", "joints3d", "joints2d", "objverts3d", "objverts2d")
POST_GRADS = ("verts_mm", "joints_mm", "scaletrans", "st_obj")
POST_SUBSETS = [(0, 1, 2, 3, 4), (0,), (1,), (2,), (3,), (4,), (2, 4), ()]
# the object rotations of a B = 6 case, one per sample (smaller batches take the first ones): zero, the tiny one, |r| = 3.1
# (near pi), |r| = 6.4 (beyond 2 pi), two random ones
_ROTATIONS = [[0.0, 0.0, 0.0], [1e-6, 0.0, 0.0], [3.1 * 0.48, 3.1 * 0.6, -3.1 * 0.64], [-6.4 * 0.8, 6.4 * 0.36, 6.4 * 0.48]]


def post_inputs(shape):
    """(verts_mm, joints_mm, scaletrans, st_obj, K, canverts) as fp32 arrays.  K per sample: fx != fy, a skew, a principal
    point away from res / 2, and in the LAST sample a third row other than (0, 0, 1)."""
    B, Vh, J, Vo = shape
    rng = np.random.default_rng(7000 + 1000 * B + Vh + 3 * J + 7 * Vo)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    verts, joints = 60.0 * rng.standard_normal((B, Vh, 3)), 60.0 * rng.standard_normal((B, J, 3))
    scaletrans, st_obj = rng.standard_normal((B, 3)), rng.standard_normal((B, 6))
    for b in range(B):
        if b < len(_ROTATIONS):
            st_obj[b, 3:] = _ROTATIONS[b]
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = 350.0 + 20.0 * rng.standard_normal(B)
    K[:, 1, 1] = 310.0 + 20.0 * rng.standard_normal(B)
    K[:, 0, 1] = 3.0 * rng.standard_normal(B)
    K[:, 0, 2] = 120.0 + 5.0 * rng.standard_normal(B)
    K[:, 1, 2] = 131.0 + 5.0 * rng.standard_normal(B)
    K[:, 2, 2] = 1.0
    K[B - 1, 2, :2] = [0.02, -0.03]
    canverts = 0.05 * rng.standard_normal((B, Vo, 3))
    return tuple(f32(a) for a in (verts, joints, scaletrans, st_obj, K, canverts))


def post_weights(shape):
    """one fixed weight tensor per output; a subset of POST_SUBSETS picks which of them enter the loss"""
    B, Vh, J, Vo = shape
    rng = np.random.default_rng(11)
    return [rng.standard_normal(s).astype(np.float32) for s in ((B, Vh, 3), (B, J, 3), (B, J, 2), (B, Vo, 3), (B, Vo, 2))]


@functools.lru_cache(maxsize=None)
def post_reference(shape, subset, dtype=torch.float64):
    """(five outputs, four gradients) of ``geom_grad_ref.post_forward`` in ``dtype``: float64 = the reference, float32 = the
    yardstick.  Treat the arrays as read-only: they are shared between tests."""
    w = post_weights(shape)
    with one_cpu_thread():
        return R.post_gradients(post_inputs(shape), POST_CONSTS, [w[k] if k in subset else None for k in range(5)], dtype)
