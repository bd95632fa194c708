"""Per-element reference gradients of the MANO layer and of the head post-processing -- TEST INFRASTRUCTURE, not product
code.  Only ``tests/`` may import this module; nothing under ``handobjectconsist_amd/`` does, and nothing here calls it.

Two references, both in float64 on the CPU:

* MANO (csrc/mano_lbs.hip): central differences of ``oracle/mano_ref.mano_forward``, one input component at a time.  Every
  operation of the layer acts per sample, so column k is perturbed for ALL samples at once and one pair of evaluations of the
  batch yields d out[b] / d x[b, k] for every b: ``2 * columns`` evaluations in all.  The outputs enter every loss the tests
  use linearly (L = <verts, w_verts> + <joints, w_joints>), so the differences are taken of the OUTPUTS once
  (``mano_jacobian``) and contracted with as many weight patterns as a test has (``mano_gradients``).
* the post-processing (csrc/meshreg_post.hip): ``post_forward`` restates meshreg/models/project.py:5-24 (recover_3d_proj),
  manopth's quaternion form of batch_rodrigues and libyana's batch_proj2d in plain torch operations; run on float64 leaves,
  autograd supplies analytic gradients for every input element.  Run on float32 tensors it is the yardstick of what an fp32
  evaluation of these formulas delivers.

``per_sample_error`` is the measure both use: every sample's largest error over that sample's largest reference entry, so a
quiet sample cannot hide behind a loud one."""
import numpy as np
import torch

from oracle import mano_ref


def central_differences(f, x, eps):
    """f: x [B, C] -> one value [B] or a vector [B, M] per sample, every sample's from that sample's row of x alone.
    -> d f[b] / d x[b, k] as [B, C] or [B, C, M], central differences in float64; column k of all samples moves at once."""
    x = np.asarray(x, np.float64)
    cols = []
    for k in range(x.shape[1]):
        d = np.zeros_like(x)
        d[:, k] = eps
        cols.append((np.asarray(f(x + d), np.float64) - np.asarray(f(x - d), np.float64)) / (2 * eps))
    return np.stack(cols, 1)


def per_sample_error(got, ref):
    """max over samples b of max |got[b] - ref[b]| / max |ref[b]|.  A sample whose reference is all zero admits no error at
    all: exact zeros give 0, anything else inf.  Empty tensors give 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    B = ref.shape[0]
    err, scale = np.abs(got - ref).reshape(B, -1).max(1), np.abs(ref).reshape(B, -1).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(rel.max())


def per_component_gradient(loss_per_sample, x, eps=1e-6):
    """-> (gradient [B, columns] of a function returning one loss per sample, the disagreement between the differences at eps
    and at 10 eps as a ``per_sample_error``).  The disagreement bounds truncation (it grows with eps) and cancellation (it
    shrinks with eps) at once: a reference is only as good as this figure."""
    grad = central_differences(loss_per_sample, x, eps)
    return grad, per_sample_error(central_differences(loss_per_sample, x, 10 * eps), grad)


# ------------------------------------------------------------------------------------------------ MANO
def _columns(pose, betas, trans):
    """[pose | betas | trans] and where each part sits.  A translation that is absent -- None, or zero for EVERY sample
    (manopth's rule) -- has no columns: perturbing it would bring it into force."""
    pose, betas = np.asarray(pose, np.float64), np.asarray(betas, np.float64)
    parts, names = [pose, betas], ["pose", "betas"]
    if trans is not None and float(np.linalg.norm(np.asarray(trans, np.float64))) != 0.0:
        parts.append(np.asarray(trans, np.float64))
        names.append("trans")
    edges = np.cumsum([0] + [p.shape[1] for p in parts])
    return np.concatenate(parts, 1), {n: slice(int(a), int(b)) for n, a, b in zip(names, edges[:-1], edges[1:])}


def mano_jacobian(c, pose, betas, trans=None, eps=1e-6, **kw):
    """d [verts | joints] / d [pose | betas | trans] per sample: ([B, columns, 778 * 3 + 21 * 3], {name: column slice}).
    ``kw``: ``use_pca``, ``center_idx``, ``ncomps`` of ``mano_ref.mano_forward``."""
    x, where = _columns(pose, betas, trans)

    def outputs(xx):
        t = xx[:, where["trans"]] if "trans" in where else None
        v, j = mano_ref.mano_forward(c, xx[:, where["pose"]], xx[:, where["betas"]], trans=t, dtype=np.float64, **kw)
        return np.concatenate([v.reshape(len(v), -1), j.reshape(len(j), -1)], 1)

    return central_differences(outputs, x, eps), where


def mano_gradients(c, pose, betas, trans, w_verts, w_joints, jacobian=None, eps=1e-6, **kw):
    """Per-sample gradients of L = <verts, w_verts> + <joints, w_joints> in float64: {"pose": [B, 18 or 48], "betas": [B, 10],
    "trans": [B, 3] or None (an absent translation)}.  ``jacobian``: what ``mano_jacobian`` returned for these inputs, to
    share the differences between weight patterns."""
    jac, where = jacobian if jacobian is not None else mano_jacobian(c, pose, betas, trans, eps=eps, **kw)
    B = jac.shape[0]
    w = np.concatenate([np.asarray(w_verts, np.float64).reshape(B, -1), np.asarray(w_joints, np.float64).reshape(B, -1)], 1)
    grad = np.einsum("bcm,bm->bc", jac, w)
    return {n: (grad[:, where[n]] if n in where else None) for n in ("pose", "betas", "trans")}


# ------------------------------------------------------------------------------------------------ head post-processing
def _recovered_centre(K, scale, trans, off_z, res):
    """project.py:14-23: Z0 = f s + off_z with f = K[0,0] ALONE; XY0 = (t + res / 2 - K[:2,2]) Z0 / f.  -> [B,3]"""
    focal = K[:, 0, 0].unsqueeze(1)
    z0 = focal * scale + off_z
    img_centre = torch.tensor([res[0] / 2, res[1] / 2], dtype=K.dtype)
    xy0 = (trans + img_centre - K[:, :2, 2]) * z0 / focal
    return torch.cat([xy0, z0], 1)


def rotation_from_axisang(r):
    """manopth rodrigues_layer.batch_rodrigues: [B,3] -> [B,3,3] through the normalised quaternion, angle = |r + 1e-8|."""
    angle = (r + 1e-8).pow(2).sum(1, keepdim=True).sqrt()
    half = angle * 0.5
    q = torch.cat([torch.cos(half), torch.sin(half) * (r / angle)], 1)
    q = q / q.pow(2).sum(1, keepdim=True).sqrt()
    w, x, y, z = q.unbind(1)
    rows = [w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
            2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
            2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def _project(points, K):
    """(K p)[:2] / (K p)[2] with the whole of K, third row included"""
    h = torch.einsum("bij,bvj->bvi", K, points)
    return h[..., :2] / h[..., 2:]


def post_forward(verts_mm, joints_mm, scaletrans, st_obj, K, canverts, trans_factor, scale_factor, off_z, res):
    """(verts_mm [B,Vh,3], joints_mm [B,J,3], scaletrans [B,3] = (s, tx, ty), st_obj [B,6] = (s, tx, ty, axis-angle), K [B,3,3],
    canverts [B,Vo,3]) -> (handverts3d, joints3d, joints2d, objverts3d, objverts2d), in the dtype of the inputs; ``res`` =
    (width, height).  Any of Vh, J, Vo may be 0."""
    c_hand = _recovered_centre(K, scaletrans[:, :1] * scale_factor, scaletrans[:, 1:] * trans_factor, off_z, res)
    handverts3d = verts_mm / 1000 + c_hand.unsqueeze(1)
    joints3d = joints_mm / 1000 + c_hand.unsqueeze(1)
    c_obj = _recovered_centre(K, st_obj[:, :1] * scale_factor, st_obj[:, 1:3] * trans_factor, off_z, res)
    rotated = torch.einsum("bij,bvj->bvi", rotation_from_axisang(st_obj[:, 3:]), canverts)
    objverts3d = rotated + c_obj.unsqueeze(1)
    return handverts3d, joints3d, _project(joints3d, K), objverts3d, _project(objverts3d, K)


def post_gradients(inputs, consts, weights, dtype):
    """Values and analytic gradients of L = sum_k <out_k, weights[k]> (``weights[k]`` None: output k unused) by autograd in
    ``dtype`` on the CPU.  ``inputs`` = (verts_mm, joints_mm, scaletrans, st_obj, K, canverts) as arrays, ``consts`` =
    (trans_factor, scale_factor, off_z, res).  -> (five outputs, gradients of the first four inputs), numpy; an input no used
    output depends on has a gradient of zeros."""
    leaves = [torch.as_tensor(np.asarray(a), dtype=dtype).clone() for a in inputs]
    for t in leaves[:4]:
        t.requires_grad_(True)
    outs = post_forward(*leaves, *consts)
    terms = [(o * torch.as_tensor(np.asarray(w), dtype=dtype)).sum() for o, w in zip(outs, weights) if w is not None]
    if terms:
        grads = torch.autograd.grad(sum(terms), leaves[:4], allow_unused=True)
    else:
        grads = [None] * 4
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves[:4])]
    return [o.detach().numpy() for o in outs], [g.numpy() for g in grads]
