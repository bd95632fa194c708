"""2-D ground truth: the reference's ``get_joints2d`` / ``get_objverts2d`` / ``get_hand_verts2d`` (ho3dv2.py:309-312, 350-354,
454-458, 500-503; fhbhands.py:361-365, 417-422, 429-432) followed by ``HandObjSet``'s mirror ``W - x``, ``transform_coords`` through
the crop affine (handobjset.py:160-225) and the cyclic padding of ``collate.pad_cyclic``.

Three kinds of point, each as base pixels (``objverts2d`` / ``handverts2d`` / ``joints2d``) and through the affine (``..._trans``):
object vertices from a model of an ``objgt.ObjectBank`` and its placement ``[A | b]`` (projected), camera-frame points
``[N,P,3]`` -- the hand's vertices -- (projected), annotated base pixels ``[N,P,2]`` -- the joints -- (taken as they are).

``points2d_host``: one sample after the other in numpy, the host path's own order of operations -- what a DataLoader worker and
``extend_collate`` do, the default path, and the device path's yardstick inside the product.  ``points2d_batch``: all frames of a
step, whatever collated dict they belong to, all kinds, in ONE ``mr_gt2d_batch`` launch after ONE upload of the
stacked records (and of whatever points came from the host); each dict's object points are padded to its own longest model,
the rule of ``objgt.obj_geometry_batch``, so ``objverts2d`` and ``objverts3d`` pad alike.

``pack_gt2d_info`` / ``unpack_gt2d_info``: a frame's intrinsics, mirror flag, width, affine and queried kinds as one float32
row, the form in which ``HandObjSet(points2d="device")`` hands them to ``assemble_batch`` (rows collate like any other array)."""
import numpy as np
import torch

from handobjectconsist_amd import _lib
from handobjectconsist_amd.datasets import handutils, manogt
from handobjectconsist_amd.utils.collate import pad_cyclic

# one row of pack_gt2d_info: K 9 | flip 1 | width 1 | affine rows 0, 1: 6 | queried keys 1
GT2D_INFO_FLOATS = 18
_K, _FLIP, _WIDTH, _AFF, _WANT = slice(0, 9), 9, 10, slice(11, 17), 17
KINDS = ("objverts2d", "handverts2d", "joints2d")
KEYS = tuple(k + s for k in KINDS for s in ("", "_trans"))
QUERY_BITS = {key: 1 << i for i, key in enumerate(KEYS)}
MAX_WIDTH = 1 << 24  # widths travel as float32
# MrGt2dRecord (include/meshraster_hip.h), in 4-byte words
RECORD_WORDS = 36
_W_MODE, _W_ROW, _W_PAD, _W_COUNT, _W_FLIP, _W_MODEL, _W_SRC = 0, 1, 2, 3, 4, 5, 6
_W_K, _W_WIDTH, _W_AFF, _W_POSE = slice(8, 17), 17, slice(18, 24), slice(24, 36)
_MODES = {"objverts2d": _lib.GT2D_BANK, "handverts2d": _lib.GT2D_POINTS3D, "joints2d": _lib.GT2D_POINTS2D}


def pack_gt2d_info(camintr, flip, width, affinetrans, queries):
    """``camintr``: the dataset's own intrinsics [3,3]; ``width``: the W of the mirror; ``affinetrans`` [3,3] (rows 0 and 1 travel:
    the last row of ``get_affine_transform``'s matrix is 0 0 1); ``queries``: any iterable of names, of which KEYS are remembered."""
    width = int(width)
    if not 0 < width < MAX_WIDTH:
        raise ValueError(f"width {width} outside 1..{MAX_WIDTH - 1}")
    camintr, affinetrans = np.asarray(camintr), np.asarray(affinetrans)
    if camintr.shape != (3, 3) or affinetrans.shape != (3, 3):
        raise ValueError(f"camintr and affinetrans must be [3,3], got {list(camintr.shape)} and {list(affinetrans.shape)}")
    row = np.zeros(GT2D_INFO_FLOATS, np.float32)
    row[_K], row[_FLIP], row[_WIDTH], row[_AFF] = camintr.reshape(9), 1.0 if flip else 0.0, width, affinetrans[:2].reshape(6)
    row[_WANT] = sum(bit for key, bit in QUERY_BITS.items() if key in queries)
    return row


def unpack_gt2d_info(rows):
    """[N, GT2D_INFO_FLOATS] -> dict(camintr [N,3,3], flip [N], width [N], affine [N,2,3], keys: the queried KEYS)."""
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 2 or rows.shape[1] != GT2D_INFO_FLOATS:
        raise ValueError(f"gt2d_info must be [N, {GT2D_INFO_FLOATS}], got {list(rows.shape)}")
    want = rows[:, _WANT]
    if len(rows) and (want.min() != want.max() or want[0] != np.floor(want[0]) or not 0 <= want[0] < 1 << len(KEYS)):
        raise ValueError("gt2d_info: the rows were packed for different queries")
    mask = int(want[0]) if len(rows) else 0
    return dict(camintr=rows[:, _K].reshape(-1, 3, 3), flip=rows[:, _FLIP] != 0, width=rows[:, _WIDTH], affine=rows[:, _AFF].reshape(-1, 2, 3),
                keys=tuple(k for k in KEYS if mask & QUERY_BITS[k]))


def project(points3d, camintr):
    """ho3dv2.py:500-503: ``camintr . p`` divided by its third component, float32."""
    hom = np.array(camintr).dot(points3d.transpose()).transpose()
    with np.errstate(divide="ignore", invalid="ignore"):
        return (hom / hom[:, 2:])[:, :2].astype(np.float32)


def _frames(camintr, flip, width, affine, groups):
    camintr = np.asarray(camintr)
    if camintr.ndim != 3 or camintr.shape[1:] != (3, 3):
        raise ValueError(f"camintr must be [N,3,3], got {list(camintr.shape)}")
    n = camintr.shape[0]
    affine = np.asarray(affine)
    if affine.shape == (n, 3, 3):
        affine = affine[:, :2]
    if affine.shape != (n, 2, 3):
        raise ValueError(f"affine must be [{n},3,3] or [{n},2,3], got {list(affine.shape)}")
    flip = np.zeros(n, bool) if flip is None else manogt._per_sample(np.asarray(flip, bool), n, (), "flip")
    width = manogt._per_sample(np.asarray(width), n, (), "width")
    if n and (width.min() < 1 or width.max() >= MAX_WIDTH or np.any(width != np.floor(width))):
        raise ValueError(f"width must be whole numbers of 1..{MAX_WIDTH - 1}")
    groups = [n] if groups is None else [int(g) for g in groups]
    if min(groups, default=0) < 0 or sum(groups) != n:
        raise ValueError(f"groups {groups} do not add up to the {n} frames")
    return camintr.astype(np.float32), flip, width.astype(np.float32), affine.astype(np.float32), groups, n


def _dense(points, n, dims, name):
    """a dense source: None, or (array or tensor [n, P, dims] with P >= 1)"""
    if points is None:
        return None
    if not torch.is_tensor(points):
        points = np.asarray(points)
    if len(points.shape) != 3 or points.shape[0] != n or points.shape[2] != dims or (n and points.shape[1] < 1):
        raise ValueError(f"{name} must be [{n}, P, {dims}] with at least one point a frame, got {list(points.shape)}")
    return points


def _sources(bank, model, pose, points3d, points2d, n):
    if (model is None) != (pose is None) or (model is not None and bank is None):
        raise ValueError("object points need a bank, model ids and placements together")
    if model is not None:
        model, pose = np.asarray(model), np.asarray(pose)
        if model.ndim != 1 or model.shape[0] != n or (model.size and not np.issubdtype(model.dtype, np.integer)):
            raise ValueError(f"model must be [{n}] integers, got {list(model.shape)} {model.dtype}")
        if pose.shape != (n, 3, 4):
            raise ValueError(f"pose must be [{n},3,4], got {list(pose.shape)}")
        bank.check_ids(model)
        model = model.astype(np.int64)
    return model, pose, _dense(points3d, n, 3, "points3d"), _dense(points2d, n, 2, "points2d")


def _only(dicts, keys):
    if keys is None:
        return dicts
    if not set(keys) <= set(KEYS):
        raise ValueError(f"keys must be among {KEYS}, got {tuple(keys)}")
    return [{k: d[k] for k in KEYS if k in keys and k in d} for d in dicts]


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else a


def points2d_host(camintr, flip, width, affine, groups=None, bank=None, model=None, pose=None, points3d=None, points2d=None, keys=None,
                  points2d_mirrored=False):
    """Per group (a collated dict's frames; one group of all frames by default) a dict of float32 numpy arrays [B,P,2]: the kinds
    whose source is given, base and ``_trans`` -- sample by sample in the host path's order of operations (handobjset.py:160-225
    on the accessors' results; the accessors in ho3dv2.py's form), object points padded with ``pad_cyclic`` to the group's longest
    model.  ``points2d`` are float32 base pixels (anything else is cast first); ``points2d_mirrored``: they carry a flipped frame's
    mirror already (the form in which ``HandObjSet`` sends the joints).  ``keys``: the keys the dicts hold (None: all of the kinds
    given)."""
    camintr, flip, width, affine, groups, n = _frames(camintr, flip, width, affine, groups)
    model, pose, points3d, points2d = _sources(bank, model, pose, points3d, points2d, n)
    points3d, points2d = _host(points3d), _host(points2d)
    per = []
    for i in range(n):
        affinetrans = np.concatenate([affine[i], np.array([[0, 0, 1]], np.float32)])
        sample = {}
        for kind, pts in (("objverts2d", None if model is None else project(bank.verts_trans(model[i], pose[i]), camintr[i])),
                          ("handverts2d", None if points3d is None else project(np.asarray(points3d[i], np.float32), camintr[i])),
                          ("joints2d", None if points2d is None else np.asarray(points2d[i], np.float32))):
            if pts is None:
                continue
            if flip[i] and not (kind == "joints2d" and points2d_mirrored):
                pts = pts.copy()
                pts[:, 0] = width[i] - pts[:, 0]
            sample[kind] = pts.astype(np.float32)
            with np.errstate(invalid="ignore"):
                sample[kind + "_trans"] = np.array(handutils.transform_coords(sample[kind], affinetrans)).astype(np.float32)
        per.append(sample)
    out, lo = [], 0
    for g in groups:
        rows = per[lo:lo + g]
        lo += g
        d = {}
        for key in (rows[0] if g else ()):
            longest = max(len(r[key]) for r in rows)
            d[key] = np.stack([pad_cyclic(r[key], longest) for r in rows])
        out.append(d)
    return _only(out, keys)


def point_records(camintr, flip, width, affine, groups=None, bank=None, model=None, pose=None, count3d=None, count2d=None,
                  points2d_mirrored=False):
    """-> (records [R, RECORD_WORDS] float32 whose integer words are int32 bit patterns (MrGt2dRecord), layout: per group a list
    of (kind, frames, padded points, first row), rows of all records together).  ``count3d`` / ``count2d``: the points a frame of
    the dense sources, or None.  Rows run group by group, inside a group kind by kind (KINDS' order), inside a kind frame by frame."""
    camintr, flip, width, affine, groups, n = _frames(camintr, flip, width, affine, groups)
    kinds = [k for k, have in zip(KINDS, (model is not None, count3d is not None, count2d is not None)) if have]
    nv = np.array([len(v) for v in bank.verts], np.int64) if model is not None else None
    rec = np.zeros((n * len(kinds), RECORD_WORDS), np.float32)
    ints = rec.view(np.int32)
    layout, lo, rows, r = [], 0, 0, 0
    for g in groups:
        blocks = []
        for kind in kinds:
            frames = np.arange(lo, lo + g)
            count = nv[model[frames]] if kind == "objverts2d" else np.full(g, count3d if kind == "handverts2d" else count2d, np.int64)
            padded = int(count.max()) if g else 0
            if rows + g * padded > 0x7fffffff:
                raise ValueError("the step's padded points have more than 2^31 - 1 rows")
            sl = slice(r, r + g)
            ints[sl, _W_MODE], ints[sl, _W_ROW], ints[sl, _W_PAD], ints[sl, _W_COUNT] = _MODES[kind], rows + padded * np.arange(g), padded, count
            ints[sl, _W_FLIP] = 0 if kind == "joints2d" and points2d_mirrored else flip[frames]
            if kind == "objverts2d":
                ints[sl, _W_MODEL] = model[frames]
                rec[sl, _W_POSE] = np.asarray(pose[frames], np.float32).reshape(g, 12)
            else:
                ints[sl, _W_SRC] = frames * count
            rec[sl, _W_K], rec[sl, _W_WIDTH], rec[sl, _W_AFF] = camintr[frames].reshape(g, 9), width[frames], affine[frames].reshape(g, 6)
            blocks.append((kind, g, padded, rows))
            rows, r = rows + g * padded, r + g
        layout.append(blocks)
        lo += g
    return rec, layout, rows


def read_records(records):
    """the fields of packed records, by name (what the kernel reads)"""
    records = np.ascontiguousarray(records, dtype=np.float32)
    ints = records.view(np.int32)
    return dict(mode=ints[:, _W_MODE], row_offset=ints[:, _W_ROW], padded=ints[:, _W_PAD], count=ints[:, _W_COUNT], flip=ints[:, _W_FLIP],
                model=ints[:, _W_MODEL], src_first=ints[:, _W_SRC], camintr=records[:, _W_K].reshape(-1, 3, 3), width=records[:, _W_WIDTH],
                affine=records[:, _W_AFF].reshape(-1, 2, 3), pose=records[:, _W_POSE].reshape(-1, 3, 4))


def run_records(records, rows, dbank=None, points3d=None, points2d=None):
    """One ``mr_gt2d_batch`` launch on the current stream: ``records`` [R, RECORD_WORDS] on the device (made dense where it is
    not), ``dbank`` from ``ObjectBank.on`` / ``finish_device_bank`` (None: no record reads a bank), ``points3d`` [..., 3] / ``points2d``
    [..., 2] device tensors (None: no record reads them) -> flat base [rows,2], trans [rows,2]."""
    _lib.check_cuda(records, points3d, points2d)
    if records.dim() != 2 or records.shape[1] != RECORD_WORDS or records.dtype != torch.float32:
        raise ValueError(f"records must be float32 [R, {RECORD_WORDS}], got {records.dtype} {list(records.shape)}")
    records = records.contiguous()
    device = records.device
    verts = table = None
    if dbank is not None:
        verts, table = _lib.contig(dbank["verts"]), _lib.contig(dbank["table"], torch.int32)
    points3d = None if points3d is None else _lib.contig(points3d).reshape(-1, 3)
    points2d = None if points2d is None else _lib.contig(points2d).reshape(-1, 2)
    if any(t is not None and t.device != device for t in (verts, table, points3d, points2d)):
        raise ValueError("the bank, the points and the records live on different devices")
    rows = int(rows)
    base = torch.empty((rows, 2), dtype=torch.float32, device=device)
    trans = torch.empty((rows, 2), dtype=torch.float32, device=device)
    P = _lib.ptr
    _lib.call("mr_gt2d_batch", P(verts), P(table), 0 if table is None else table.shape[0], 0 if verts is None else verts.shape[0],
              P(points3d), 0 if points3d is None else points3d.shape[0], P(points2d), 0 if points2d is None else points2d.shape[0],
              P(records), records.shape[0], rows, P(base), P(trans), rows, _lib.stream_ptr(device))
    return base, trans


def points2d_batch(camintr, flip, width, affine, groups=None, bank=None, model=None, pose=None, points3d=None, points2d=None, device="cuda",
                   keys=None, points2d_mirrored=False):
    """``points2d_host`` for all frames of a step in one launch: per group a dict of tensors on ``device`` (views of two flat
    buffers).  The stacked records -- and the dense points that are host arrays -- travel in one host-to-device copy; the bank is
    resident; dense points that are tensors must live on ``device`` already (the hand's vertices, where ``forward_full`` left
    them).  No frame: empty dicts' worth of tensors, no launch.  ``keys``: the keys the dicts hold (None: all of the kinds given;
    the launch writes base and ``_trans`` either way)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("points2d_batch runs on a GPU; points2d_host is the host path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    _only([], keys)
    camintr, flip, width, affine, groups, n = _frames(camintr, flip, width, affine, groups)  # (every check before any upload)
    model, pose, points3d, points2d = _sources(bank, model, pose, points3d, points2d, n)
    for name, t in (("points3d", points3d), ("points2d", points2d)):
        if torch.is_tensor(t) and t.device != device:
            raise ValueError(f"{name} lives on {t.device}, the bank and the outputs on {device}: the points and the bank must share a device")
        if torch.is_tensor(t) and t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    records, layout, rows = point_records(camintr, flip, width, affine, groups, bank, model, pose,
                                          None if points3d is None else points3d.shape[1], None if points2d is None else points2d.shape[1],
                                          points2d_mirrored)
    if n == 0 or rows == 0:
        empty = lambda: torch.empty((0, 0, 2), dtype=torch.float32, device=device)
        return _only([{k + s: empty() for k, *_ in blocks for s in ("", "_trans")} for blocks in layout], keys)
    dbank = bank.on(device) if model is not None else None
    parts = [records] + [np.ascontiguousarray(p, dtype=np.float32) for p in (points3d, points2d) if p is not None and not torch.is_tensor(p)]
    buf = torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).to(device, non_blocking=True)
    views, lo = [], 0
    for p in parts:  # (contiguous views of the one upload: every block starts on a float)
        views.append(buf[lo:lo + p.size].view(p.shape))
        lo += p.size
    rest = iter(views[1:])
    points3d = points3d if points3d is None or torch.is_tensor(points3d) else next(rest)
    points2d = points2d if points2d is None or torch.is_tensor(points2d) else next(rest)
    base, trans = run_records(views[0], rows, dbank, points3d, points2d)
    out = []
    for blocks in layout:
        d = {}
        for kind, g, padded, first in blocks:
            d[kind], d[kind + "_trans"] = (t[first:first + g * padded].view(g, padded, 2) for t in (base, trans))
        out.append(d)
    return _only(out, keys)


def hand_cam_verts(layer, fullpose, shape, trans, cam_rot=None, device="cuda"):
    """The hand's vertices in the camera frame, [N,778,3] float32 on ``device``: what the dataset's ``get_hand_verts3d`` returns
    (fhbhands.py:355-359, ho3dv2.py:341-348) BEFORE ``HandObjSet`` mirrors, rotates and centres them -- one ``forward_full`` call
    whose epilogue holds only the scale to metres, the annotated translation and the camera rotation."""
    fullpose, shape, trans, n = manogt._check(fullpose, shape, trans)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("hand_cam_verts runs on a GPU; the dataset's get_hand_verts3d is the host path")
    cam_rot = manogt._per_sample(cam_rot, n, (3, 3), "cam_rot")
    if n == 0:
        return torch.empty((0, 778, 3), dtype=torch.float32, device=device)
    parts = [fullpose, shape, trans] + ([np.asarray(cam_rot, np.float32)] if cam_rot is not None else [])
    flat = np.concatenate([np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in parts])
    buf = torch.from_numpy(flat).to(device, non_blocking=True)
    views, lo = [], 0
    for p in parts:
        views.append(buf[lo:lo + p.size].view(p.shape))
        lo += p.size
    post = {"scale": 1.0 / 1000.0, "trans": views[2]}
    if cam_rot is not None:
        post["rot"] = views[3]
    verts, _ = manogt._layer_on(layer, device).forward_full(views[0], views[1], post=post)
    return verts
