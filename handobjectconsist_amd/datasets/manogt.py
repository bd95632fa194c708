"""Ground-truth hand meshes from MANO annotations: the reference's ``get_hand_verts3d`` (fhbhands.py:355-359,
ho3dv2.py:341-348) followed by ``HandObjSet``'s mirror / rotate / centre (handobjset.py:160-182).

``hand_verts_host``: one sample after the other through ``SynthManoLayer.forward_torch`` on the CPU at batch size 1, the
reference's own order of operations -- what a DataLoader worker does, the default path, and the device path's yardstick inside
the product.  ``hand_verts_batch``: all frames of a step in ONE call of ``SynthManoLayer.forward_full`` on the GPU
(mr_mano_forward_full) after ONE upload of the stacked annotations; the scale to metres, the annotated translation,
the camera rotation, the mirror, the augmentation rotation and the centre subtraction are the kernel's rigid epilogue.

``pack_hand_info`` / ``unpack_hand_info``: a sample's annotation and transform as one float32 row, the form in which
``HandObjSet(hand_geometry="device")`` hands them to ``assemble_batch`` (rows collate like any other array)."""
import copy
import weakref

import numpy as np
import torch

# one row of pack_hand_info: fullpose 48 | shape 10 | trans 3 | flip 1 | rot_mat 9 | has_center 1 | center3d 3 | has_cam 1 | cam_rot 9
HAND_INFO_FLOATS = 85
_POSE, _SHAPE, _TRANS, _FLIP, _ROT, _HASC, _C3D, _HASCAM, _CAM = (
    slice(0, 48), slice(48, 58), slice(58, 61), 61, slice(62, 71), 71, slice(72, 75), 75, slice(76, 85))


def pack_hand_info(fullpose, trans, shape, flip=False, rot_mat=None, center3d=None, cam_rot=None):
    row = np.zeros(HAND_INFO_FLOATS, np.float32)
    row[_POSE], row[_SHAPE], row[_TRANS] = np.asarray(fullpose).reshape(48), np.asarray(shape).reshape(10), np.asarray(trans).reshape(3)
    row[_FLIP] = 1.0 if flip else 0.0
    row[_ROT] = (np.eye(3) if rot_mat is None else np.asarray(rot_mat)).reshape(9)
    if center3d is not None:
        row[_HASC], row[_C3D] = 1.0, np.asarray(center3d).reshape(3)
    if cam_rot is not None:
        row[_HASCAM], row[_CAM] = 1.0, np.asarray(cam_rot).reshape(9)
    return row


def unpack_hand_info(rows):
    """[N, HAND_INFO_FLOATS] -> the keyword arguments of ``hand_verts_batch`` / ``hand_verts_host``."""
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 2 or rows.shape[1] != HAND_INFO_FLOATS:
        raise ValueError(f"hand_info must be [N, {HAND_INFO_FLOATS}], got {list(rows.shape)}")
    for name, col in (("center3d", _HASC), ("cam_rot", _HASCAM)):
        if rows[:, col].min() != rows[:, col].max():
            raise ValueError(f"hand_info: some rows carry {name} and some do not")
    return dict(fullpose=rows[:, _POSE], shape=rows[:, _SHAPE], trans=rows[:, _TRANS], flip=rows[:, _FLIP] != 0,
                rot_mat=rows[:, _ROT].reshape(-1, 3, 3), center3d=rows[:, _C3D] if rows[0, _HASC] else None,
                cam_rot=rows[:, _CAM].reshape(-1, 3, 3) if rows[0, _HASCAM] else None)


def _per_sample(a, n, shape, name):
    """``a`` as [n, *shape]: one value for all samples, or one per sample."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.shape == shape:
        a = np.broadcast_to(a, (n,) + shape)
    if a.shape != (n,) + shape:
        raise ValueError(f"{name} must be {list(shape)} or {[n] + list(shape)}, got {list(a.shape)}")
    return a


def _check(fullpose, shape, trans):
    fullpose, shape, trans = np.asarray(fullpose), np.asarray(shape), np.asarray(trans)
    n = fullpose.shape[0]
    if fullpose.ndim != 2 or shape.shape != (n, 10) or trans.shape != (n, 3):
        raise ValueError(f"fullpose [N, P], shape [N,10], trans [N,3] expected, got {list(fullpose.shape)}, {list(shape.shape)}, "
                         f"{list(trans.shape)}")
    return fullpose, shape, trans, n


def hand_verts_host(layer, fullpose, shape, trans, cam_rot=None, flip=None, rot_mat=None, center3d=None):
    """[N,778,3] float32 on the host, sample by sample, in the reference's order of operations.  ``layer``: a CPU
    ``SynthManoLayer`` (the datasets build ``use_pca=False, flat_hand_mean=True, center_idx=None``)."""
    fullpose, shape, trans, n = _check(fullpose, shape, trans)
    cam_rot, rot_mat = _per_sample(cam_rot, n, (3, 3), "cam_rot"), _per_sample(rot_mat, n, (3, 3), "rot_mat")
    center3d = _per_sample(center3d, n, (3,), "center3d")
    flip = None if flip is None else _per_sample(np.asarray(flip, bool), n, (), "flip")
    out = np.empty((n, 778, 3), np.float32)
    for i in range(n):
        with torch.no_grad():
            verts, _ = layer.forward_torch(torch.Tensor(fullpose[i]).unsqueeze(0), torch.Tensor(shape[i]).unsqueeze(0))
        verts = verts[0].numpy() / 1000 + trans[i]                      # fhbhands.py:358, ho3dv2.py:346
        if cam_rot is not None:
            verts = cam_rot[i].dot(verts.transpose()).transpose()       # ho3dv2.py:347
        pts = np.array(verts, dtype=np.float32)                         # handobjset.py:160-164 (mirrored)
        if flip is not None and flip[i]:
            pts[:, 0] = -pts[:, 0]
        if rot_mat is not None:
            pts = np.asarray(rot_mat[i], np.float32).dot(pts.transpose(1, 0)).transpose()  # :166-167 (rotated)
        out[i] = (pts - center3d[i] if center3d is not None else pts).astype(np.float32)   # :182
    return out


_device_layers = weakref.WeakKeyDictionary()  # layer -> {device: (key of the layer's buffers, its copy there)}


def _layer_on(layer, device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if layer.th_v_template.device == device:
        return layer
    # the key of hip_constants(): the copy is made again if the layer's buffers move or are overwritten (load_state_dict of
    # other MANO weights after a first call) or its settings change
    key = (layer.ncomps, layer.center_idx, layer.use_pca) + tuple((b.data_ptr(), b._version) for b in layer.buffers())
    copies = _device_layers.setdefault(layer, {})
    if device not in copies or copies[device][0] != key:
        copies[device] = (key, copy.deepcopy(layer).to(device))
    return copies[device][1]


def fold_transform(n, cam_rot=None, flip=None, rot_mat=None):
    """The rotation the epilogue applies after ``verts / 1000 + trans``: camera rotation, then the mirror (x negated), then
    the augmentation rotation -- the host code's order -- as one [n,3,3] float32 matrix.  Mirror and a float32 ``rot_mat``
    fold exactly (sign flips of a column); a camera rotation is multiplied in float64 and rounded once."""
    rot = np.broadcast_to(np.eye(3), (n, 3, 3)).astype(np.float64) if rot_mat is None else np.asarray(rot_mat, np.float32).astype(np.float64)
    rot = rot.copy()
    if flip is not None:
        rot[np.asarray(flip, bool), :, 0] *= -1.0
    if cam_rot is not None:
        rot = np.matmul(rot, np.asarray(cam_rot, np.float64))
    return rot.astype(np.float32)


def hand_verts_batch(layer, fullpose, shape, trans, cam_rot=None, flip=None, rot_mat=None, center3d=None, device="cuda"):
    """``hand_verts_host`` for all N frames of a step in one ``forward_full`` call: [N,778,3] float32 on ``device``.  The
    stacked annotations and the folded per-sample transform travel in one host-to-device copy."""
    fullpose, shape, trans, n = _check(fullpose, shape, trans)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("hand_verts_batch runs on a GPU; hand_verts_host is the host path")
    cam_rot, rot_mat = _per_sample(cam_rot, n, (3, 3), "cam_rot"), _per_sample(rot_mat, n, (3, 3), "rot_mat")
    center3d = _per_sample(center3d, n, (3,), "center3d")
    flip = None if flip is None else _per_sample(np.asarray(flip, bool), n, (), "flip")
    if n == 0:
        return torch.empty((0, 778, 3), dtype=torch.float32, device=device)
    parts = [fullpose, shape, trans, fold_transform(n, cam_rot, flip, rot_mat)] + ([center3d] if center3d is not None else [])
    flat = np.concatenate([np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in parts])
    buf = torch.from_numpy(flat).to(device, non_blocking=True)
    views, lo = [], 0
    for p in parts:  # (contiguous views of the one upload: every block starts on a float)
        views.append(buf[lo:lo + p.size].view(p.shape))
        lo += p.size
    post = {"scale": 1.0 / 1000.0, "trans": views[2], "rot": views[3]}
    if center3d is not None:
        post["trans2"] = views[4]
    verts, _ = _layer_on(layer, device).forward_full(views[0], views[1], post=post)
    return verts
