"""Hand-object frame sequences -> samples for the consistency trainer; counterpart of
meshreg/datasets/handobjset.py (same constructor arguments, same augmentation draws, same sequence
sampling) re-cut for a GPU-side image path:

* a sample carries the DECODED frame (uint8 HWC) together with its crop affine and flip flag instead of the
  transformed image; ``assemble_batch`` uploads the collated frames and produces ``image`` / ``jittermask``
  for the whole batch with one kernel (``frames.frames_to_batch``, bit-exact with the PIL path of
  handobjset.py:361-379);
* samples are dicts keyed by plain strings (the names of the reference's query enums in lower case:
  TransQueries.IMAGE -> "image", TransQueries.JITTERMASK -> "jittermask", TransQueries.CAMINTR -> "camintr",
  TransQueries.JOINTS3D -> "joints3d", TransQueries.HANDVERTS3D -> "handverts3d", TransQueries.OBJVERTS3D ->
  "objverts3d", BaseQueries.OBJFACES -> "objfaces", BaseQueries.OBJCANVERTS -> "objcanverts", ...).

``pose_dataset`` is any object with the accessor protocol of the reference's dataset classes
(ho3dv2.py / fhbhands.py): get_image, get_center_scale, get_camintr, get_joints3d, get_hand_verts3d,
get_obj_verts_trans, get_obj_faces, get_obj_verts_can, get_sides, get_dist_idx.  Colour jitter and blur
(libyana colortrans + PIL filters on the host, handobjset.py:339-358) are a host callable: ``datasets/coloraugm.py``
by default (blur pinned by a fixture, jitter restated), ``color_fn=None`` switches them off.  ``color_fn="device"``: the same
draws, applied by ``assemble_batch`` on the GPU (``frames.color_augment``, byte for byte Pillow's result): the sample then
carries the untouched frame and its ``color_plan``.  ``decode="device"`` (needs ``pose_dataset.get_image_bytes``): the sample
carries the JPEG file's entropy-decoded PACKED FRAME as ``frame_jpeg`` instead of ``frame``; ``assemble_batch`` uploads the
stacked packed frames once and reconstructs the pixels on the GPU (``jpegdecode.reconstruct``, byte for byte Pillow's decode).
A file that starts with the PNG signature travels as ``frame_png`` instead: its inflated, still filtered scanlines
(``pngdecode.inflate``), which ``assemble_batch`` unfilters on the GPU (``pngdecode.unfilter``).
``hand_geometry="device"`` (needs ``pose_dataset.get_hand_info``): the sample carries the frame's MANO annotation and its small
transform (flip, rotation, centre) as one ``hand_info`` row (``manogt.pack_hand_info``) instead of ``handverts3d``;
``assemble_batch`` evaluates the layer for all frames of the step in one GPU call (``manogt.hand_verts_batch``).
``hand_cam_rot`` (3x3, only with ``hand_geometry="device"``): the rotation the dataset's ``get_hand_verts3d`` applies after the
translation (ho3dv2.py:347: ``cam_extr[:3, :3]``); None for a dataset that applies none (fhbhands.py:355-359, which HAS a
``cam_extr`` and does not use it for the hand).  It is the caller's statement about the dataset: no attribute is read.
``frame_size`` ((W, H), or None): the frame size the pose dataset's centre, scale, intrinsics and 2-D annotations refer to
(fhbhands.py:110-130 reads quarter-size copies and scales its annotations by ``reduce_factor``).  Files of another size are
resized to it with Pillow's BILINEAR ``Image.resize`` in front of the colour path: by ``get_sample`` on the host, or
(``decode="device"``) by ``assemble_batch`` on the GPU between the decode and ``color_augment`` (``frames.resize``, byte for byte
the same) -- the sample then carries ``resize_to``.  Files of that size, and None, change nothing.
``obj_geometry="device"`` (needs ``pose_dataset.get_obj_info(idx) -> (model id, pose [3,4])``): the sample carries the frame's
model id, its placement ``[A | b]`` and the same small transform as one ``obj_info`` row (``objgt.pack_obj_info``) instead of
``objverts3d`` / ``objfaces`` / ``objcanverts`` / ``objcantrans`` / ``objcanscale`` (the row remembers which of the three object queries were asked for: the batch gets the keys
the host path would have given it); ``assemble_batch(obj_bank=...)`` gathers them
from the device-resident model bank for all frames of the step in one GPU call (``objgt.obj_geometry_batch``).
The 2-D queries (none of them a default): ``affinetrans`` (TransQueries.AFFINETRANS), ``joints2d`` / ``objverts2d`` / ``handverts2d``
(BaseQueries: ``pose_dataset.get_joints2d`` / ``get_objverts2d`` / ``get_hand_verts2d``, x mirrored as ``W - x`` where the hand is
flipped, W the frame's width) and the same with ``_trans`` (TransQueries: through ``affinetrans``), handobjset.py:160-225.  They
need ``frame`` among the queries: the affine and W are the frame's.  ``points2d="device"``: the sample carries one ``gt2d_info`` row
(``gt2d.pack_gt2d_info``: the dataset's intrinsics, flip, W, the affine, the queried keys) and the annotated joints' base pixels
(``gt2d_joints``) instead; ``assemble_batch`` projects, mirrors and crops the resident meshes for all frames of the step in one GPU
call (``gt2d.points2d_batch``).  ``objverts2d`` then needs ``obj_geometry="device"`` and one of its three queries (the
``obj_info`` row carries the model and the placement), ``handverts2d`` needs ``hand_geometry="device"`` and ``handverts3d`` (the
``hand_info`` row carries the annotation)."""
import random
import traceback

import numpy as np
import torch
from torch.distributions.normal import Normal
from torch.distributions.uniform import Uniform
from torch.utils.data import Dataset

from handobjectconsist_amd.datasets import framecodec
from handobjectconsist_amd.datasets import frames as frames_mod
from handobjectconsist_amd.datasets import handutils

DEFAULT_QUERIES = ("frame", "camintr", "joints3d", "handverts3d", "objverts3d", "objfaces", "objcanverts", "side")
# the 2-D ground truth: kind -> the pose dataset's accessor (handobjset.py:160-225's order)
POINTS2D_GETTERS = (("joints2d", "get_joints2d"), ("objverts2d", "get_objverts2d"), ("handverts2d", "get_hand_verts2d"))
POINTS2D_KEYS = tuple(k + s for k, _ in POINTS2D_GETTERS for s in ("", "_trans"))


def flip_hand_side(target_side, hand_side):
    """datutils.flip_hand_side (datutils.py:1-12): mirror left hands to right (or the opposite) on request."""
    if target_side in ("right", "left") and hand_side != target_side:
        return target_side, True
    return hand_side, False


class HandObjSet(Dataset):
    def __init__(self, pose_dataset, center_idx=9, inp_res=(256, 256), max_rot=np.pi, normalize_img=False,
                 split="train", scale_jittering=0.3, center_jittering=0.2, train=True, hue=0.15, saturation=0.5,
                 contrast=0.5, brightness=0.5, blur_radius=0.5, spacing=2, queries=DEFAULT_QUERIES, sides="both",
                 block_rot=False, sample_nb=None, has_dist2strong=False, color_fn="reference", decode="host",
                 hand_geometry="host", hand_cam_rot=None, frame_size=None, obj_geometry="host", points2d="host"):
        if obj_geometry not in ("host", "device"):
            raise ValueError(f"obj_geometry must be 'host' or 'device', got {obj_geometry!r}")
        if obj_geometry == "device" and not hasattr(pose_dataset, "get_obj_info"):
            raise ValueError("obj_geometry=\"device\" needs a pose_dataset with get_obj_info(idx) (model id, pose [3,4])")
        self.obj_geometry = obj_geometry
        if hand_geometry not in ("host", "device"):
            raise ValueError(f"hand_geometry must be 'host' or 'device', got {hand_geometry!r}")
        if hand_geometry == "device" and not hasattr(pose_dataset, "get_hand_info"):
            raise ValueError("hand_geometry=\"device\" needs a pose_dataset with get_hand_info(idx) (fullpose, trans, shape)")
        if hand_cam_rot is not None:
            if hand_geometry != "device":
                raise ValueError("hand_cam_rot states what get_hand_verts3d does, for hand_geometry=\"device\"; the host path calls "
                                 "get_hand_verts3d itself and would ignore it")
            hand_cam_rot = np.array(hand_cam_rot, dtype=np.float32)
            if hand_cam_rot.shape != (3, 3):
                raise ValueError(f"hand_cam_rot must be a 3x3 rotation (cam_extr[:3, :3]), got {list(hand_cam_rot.shape)}")
        self.hand_geometry, self.hand_cam_rot = hand_geometry, hand_cam_rot
        if decode not in ("host", "device"):
            raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
        if decode == "device":
            if color_fn not in ("device", None):
                raise ValueError("decode=\"device\" leaves no pixels on the host: color_fn must be \"device\" or None")
            if not hasattr(pose_dataset, "get_image_bytes"):
                raise ValueError("decode=\"device\" needs a pose_dataset with get_image_bytes(idx) (the JPEG or PNG file's bytes)")
        self.decode = decode
        if frame_size is not None:
            if len(tuple(frame_size)) != 2 or min(int(v) for v in frame_size) < 1:
                raise ValueError(f"frame_size must be (W, H) with sides of at least 1, got {frame_size!r}")
            frame_size = (int(frame_size[0]), int(frame_size[1]))
        self.frame_size = frame_size
        self.pose_dataset = pose_dataset
        self.center_idx, self.inp_res = center_idx, tuple(inp_res)
        self.normalize_img, self.sides = normalize_img, sides
        self.sample_nb, self.spacing = sample_nb, spacing
        self.hue, self.contrast, self.brightness, self.saturation = hue, contrast, brightness, saturation
        self.blur_radius = blur_radius
        self.max_rot, self.block_rot = max_rot, block_rot
        self.train, self.scale_jittering, self.center_jittering = train, scale_jittering, center_jittering
        self.queries = tuple(queries)
        if points2d not in ("host", "device"):
            raise ValueError(f"points2d must be 'host' or 'device', got {points2d!r}")
        self.points2d = points2d
        for kind, getter in POINTS2D_GETTERS:
            if kind not in self.queries and kind + "_trans" not in self.queries:
                continue
            if "frame" not in self.queries:
                raise ValueError(f"{kind}: the 2-D queries need \"frame\" among the queries (the crop affine and the mirror's width are the frame's)")
            if points2d == "host" or kind == "joints2d":
                if not hasattr(pose_dataset, getter):
                    raise ValueError(f"the query {kind!r} needs a pose_dataset with {getter}(idx)")
            elif kind == "objverts2d" and (obj_geometry != "device" or not any(k in self.queries for k in ("objverts3d", "objfaces", "objcanverts"))):
                raise ValueError("points2d=\"device\": objverts2d needs obj_geometry=\"device\" and one of objverts3d / objfaces / objcanverts among "
                                 "the queries (their obj_info row carries the model and the placement)")
            elif kind == "handverts2d" and (hand_geometry != "device" or "handverts3d" not in self.queries):
                raise ValueError("points2d=\"device\": handverts2d needs hand_geometry=\"device\" and handverts3d among the queries (its hand_info "
                                 "row carries the annotation)")
        self.has_dist2strong = has_dist2strong
        if color_fn == "reference":  # the reference's own augmentation (handobjset.py:339-358)
            from handobjectconsist_amd.datasets import coloraugm

            color_fn = coloraugm.make_color_fn(jitter=True)
        elif color_fn == "device":  # the same draws; the pixels are done on the GPU by assemble_batch
            from handobjectconsist_amd.datasets import coloraugm

            color_fn = coloraugm.make_color_fn(jitter=True, apply="device")
        # (frame_u8, dataset, color_augm | None, blur_radius) -> (frame_u8, color_augm[, color_plan of a device path])
        self.color_fn = color_fn

    def __len__(self):
        return len(self.pose_dataset)

    # ---- augmentation draws (handobjset.py:130-157): same distributions, same order of draws
    def draw_space_augm(self, center, scale):
        if not self.train:
            return {"rot": 0, "scale": scale, "center": center}
        center_jit = Uniform(low=-1, high=1).sample((2,)).numpy()
        center = center + (self.center_jittering * scale * center_jit).astype(int)
        scale_jit = Normal(0, 1).sample().item() + 1
        factor = np.clip(self.scale_jittering * scale_jit, 1 - self.scale_jittering, 1 + self.scale_jittering)
        rot = Uniform(low=-self.max_rot, high=self.max_rot).sample().item()
        return {"rot": rot, "scale": scale * factor, "center": center}

    def get_sample(self, idx, query=None, color_augm=None, space_augm=None):
        ds, q = self.pose_dataset, (self.queries if query is None else query)
        sample = {}
        hand_side, flip = flip_hand_side(self.sides, ds.get_sides(idx)) if "side" in q else (None, False)
        if hand_side is not None:
            sample["side"] = hand_side
        want_img = "frame" in q
        if want_img:
            center, scale = ds.get_center_scale(idx)
            if self.decode == "device":
                data = ds.get_image_bytes(idx)
                codec = framecodec.codec_for(data)
                frame, packed = None, codec.host_stage(data)
                info = codec.packed_info(packed)  # (the file's own size, as its headers give it: no second parse)
                width = info["width"]
                if self.frame_size is not None and (width, info["height"]) != self.frame_size:
                    # the packed frame travels as it is; assemble_batch resizes after the decode
                    sample["resize_to"] = np.array(self.frame_size, dtype=np.int32)
                    width = self.frame_size[0]
            else:
                frame = np.asarray(ds.get_image(idx))
                if self.frame_size is not None and (frame.shape[1], frame.shape[0]) != self.frame_size:
                    from PIL import Image

                    frame = np.asarray(Image.fromarray(frame).resize(self.frame_size, Image.BILINEAR))
                width = frame.shape[1]
            if flip:
                center = np.array(center).copy()
                center[0] = width - center[0]
            if space_augm is None:
                space_augm = self.draw_space_augm(center, scale)
        elif space_augm is None:
            space_augm = {"rot": 0, "scale": None, "center": None}
        rot = 0 if self.block_rot else space_augm["rot"]
        space_augm = dict(space_augm, rot=rot)
        sample["space_augm"] = space_augm
        rot_mat = np.array([[np.cos(rot), -np.sin(rot), 0], [np.sin(rot), np.cos(rot), 0], [0, 0, 1]]).astype(np.float32)
        if want_img:
            affinetrans, post_rot_trans = handutils.get_affine_transform(space_augm["center"], space_augm["scale"],
                                                                        self.inp_res, rot=rot)
            sample["affinetrans"] = affinetrans
            if self.train:
                # the blur radius is drawn for EVERY training frame, also for the companions of a sequence that inherit
                # their colour parameters (handobjset.py:341): part of how far a sample advances torch's RNG stream
                blur_radius = Uniform(low=0, high=1).sample().item() * self.blur_radius
                if self.color_fn is not None and frame is None:
                    # the packed frame travels as it is: only the draws happen here (a device colour path never reads pixels)
                    _, color_augm, *plan = self.color_fn(None, self, color_augm, blur_radius)
                    sample["color_plan"] = plan[0]
                elif self.color_fn is not None:
                    # (the reference blurs the MIRRORED image, handobjset.py:120-122 before :341; the frame travels unmirrored
                    # to the GPU kernel, which flips on the fly: mirror, augment, mirror back, the reference's order of
                    # operations kept as it is.  Blur and jitter are mirror-symmetric to the last bit -- each blur case of
                    # tests/test_oracle_coloraugm.py also runs mirrored -- which is why a device plan carries no flip)
                    view = frame[:, ::-1] if flip else frame
                    view, color_augm, *plan = self.color_fn(view, self, color_augm, blur_radius)
                    if plan:
                        sample["color_plan"] = plan[0]
                    frame = view[:, ::-1] if flip else view
            sample["color_augm"] = color_augm if self.train else None
            if frame is None:
                sample[codec.key] = packed
            else:
                sample["frame"] = np.ascontiguousarray(frame)
            sample["flip"] = bool(flip)
        want2d = [(kind, getter) for kind, getter in POINTS2D_GETTERS if kind in q or kind + "_trans" in q]
        if want2d and not want_img:
            raise ValueError("the 2-D queries need \"frame\" among the queries")
        if want2d and self.points2d == "device":
            # the intrinsics, the mirror and the affine travel; the meshes are projected on the GPU by assemble_batch
            from handobjectconsist_amd.datasets import gt2d

            sample["gt2d_info"] = gt2d.pack_gt2d_info(ds.get_camintr(idx), flip, width, affinetrans, q)
        for kind, getter in want2d:
            if self.points2d == "device" and kind != "joints2d":
                continue
            pts = getattr(ds, getter)(idx)
            if flip:
                pts = pts.copy()
                pts[:, 0] = width - pts[:, 0]
            if self.points2d == "device":
                sample["gt2d_joints"] = pts.astype(np.float32)  # (the annotated joints: base pixels, mirrored already)
                continue
            if kind in q:
                sample[kind] = pts.astype(np.float32)
            if kind + "_trans" in q:
                sample[kind + "_trans"] = np.array(handutils.transform_coords(pts, affinetrans)).astype(np.float32)
        if "camintr" in q:
            camintr = ds.get_camintr(idx)
            # the rotation is applied to the 3-D annotations: only the crop multiplies the intrinsics (:180-183)
            sample["camintr"] = (post_rot_trans.dot(camintr) if want_img else camintr).astype(np.float32)

        def mirrored(pts):
            pts = np.array(pts, dtype=np.float32)
            if flip:
                pts[:, 0] = -pts[:, 0]
            return pts

        def rotated(pts):
            return rot_mat.dot(pts.transpose(1, 0)).transpose()

        center3d = None
        if any(k in q for k in ("joints3d", "handverts3d", "objverts3d")):
            joints3d = mirrored(ds.get_joints3d(idx))
            if self.train:
                joints3d = rotated(joints3d)
            if self.center_idx is not None:
                center3d = (joints3d[9] + joints3d[0]) / 2 if self.center_idx == -1 else joints3d[self.center_idx]
            if "joints3d" in q:
                sample["joints3d"] = (joints3d - center3d if center3d is not None else joints3d).astype(np.float32)
            sample["center3d"] = None if center3d is None else center3d.astype(np.float32)
        for key, getter in (("handverts3d", "get_hand_verts3d"), ("objverts3d", "get_obj_verts_trans")):
            if key in q:
                if key == "handverts3d" and self.hand_geometry == "device":
                    # the annotation travels; the mesh is evaluated on the GPU by assemble_batch (same mirror, rotation, centre)
                    from handobjectconsist_amd.datasets import manogt

                    pose, trans, shape = ds.get_hand_info(idx)
                    sample["hand_info"] = manogt.pack_hand_info(pose, trans, shape, flip=flip, rot_mat=rot_mat, center3d=center3d,
                                                                cam_rot=self.hand_cam_rot)
                    continue
                if key == "objverts3d" and self.obj_geometry == "device":
                    continue
                pts = rotated(mirrored(getattr(ds, getter)(idx)))
                sample[key] = (pts - center3d if center3d is not None else pts).astype(np.float32)
        if self.obj_geometry == "device":
            if any(k in q for k in ("objverts3d", "objfaces", "objcanverts")):
                # the model's id and placement travel; the meshes are gathered on the GPU by assemble_batch (same mirror, rotation, centre)
                from handobjectconsist_amd.datasets import objgt

                model, pose34 = ds.get_obj_info(idx)
                sample["obj_info"] = objgt.pack_obj_info(model, pose34, flip=flip, rot_mat=rot_mat, center3d=center3d, queries=q)
            return sample
        if "objfaces" in q:
            sample["objfaces"] = np.asarray(ds.get_obj_faces(idx))
        if "objcanverts" in q:
            canverts, cantrans, canscale = ds.get_obj_verts_can(idx)
            sample["objcanverts"] = mirrored(canverts)
            sample["objcanscale"], sample["objcantrans"] = canscale, cantrans
        return sample

    def get_safesample(self, idx, color_augm=None, space_augm=None):
        """A frame that fails to load is replaced by a neighbour within +-10 (handobjset.py:386-394)."""
        try:
            return self.get_sample(idx, color_augm=color_augm, space_augm=space_augm)
        except Exception:
            traceback.print_exc()
            other = random.randint(max(0, idx - 10), min(len(self), idx + 10))
            print(f"Encountered error processing sample {idx}, trying {other} instead")
            return self.get_sample(other)

    def sequence_offsets(self):
        """Signed frame distances of the sample_nb - 1 companions, as the reference's loop produces them
        (handobjset.py:404-418; the distance grows on both branches): +s, -s, +3s, -3s, +5s, ..."""
        offs, dist = [], 0
        for k in range((self.sample_nb or 1) - 1):
            if k % 2 == 0:
                dist += self.spacing
                offs.append(dist)
            else:
                offs.append(-dist)
                dist += self.spacing
        return offs

    def __getitem__(self, idx):
        sample = self.get_safesample(idx)
        sample["dist2query"] = 0
        space_augm, color_augm = sample.pop("space_augm"), sample.pop("color_augm", None)
        if self.sample_nb is None:
            return sample
        samples = [sample]
        for off in self.sequence_offsets():
            next_idx, dist2query = self.pose_dataset.get_dist_idx(idx, dist=off)
            # companions share the augmentation of the query frame so that photometric consistency holds
            other = self.get_safesample(next_idx, color_augm=color_augm, space_augm=space_augm)
            other["dist2query"] = dist2query
            other.pop("space_augm")
            other.pop("color_augm", None)
            samples.append(other)
        return samples


def _stack_rows(rows):
    """Per-dict tensors ([frames, ...] each) -> one tensor over all frames of the step, and ``split``: a result with one row
    per frame -> the list of each dict's rows of it."""
    bounds = np.cumsum([0] + [len(r) for r in rows])
    return torch.cat(rows, 0), lambda result: [result[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:])]


def _hand_verts(dicts, outs, device, mano_layer):
    """The dicts' ``hand_info`` rows -> ``handverts3d`` in ``outs``, through one ``manogt.hand_verts_batch`` call."""
    with_info = sum("hand_info" in d for d in dicts)
    if not with_info:
        return
    if with_info != len(dicts):
        raise ValueError(f"hand_info in {with_info} of {len(dicts)} dicts: a batch mixes samples of "
                         "HandObjSet(hand_geometry=\"device\") with samples that carry their vertices")
    if mano_layer is None:
        raise ValueError("hand_info needs assemble_batch(mano_layer=...): the layer the annotations are evaluated with")
    from handobjectconsist_amd.datasets import manogt

    rows = [torch.as_tensor(np.asarray(d["hand_info"], np.float32)) for d in dicts]
    if any(r.dim() != 2 for r in rows):
        raise ValueError("hand_info must be collated: [frames, values] per dict, not one sample's row")
    infos, split = _stack_rows(rows)
    verts = manogt.hand_verts_batch(mano_layer, device=device, **manogt.unpack_hand_info(infos.numpy()))
    for o, v in zip(outs, split(verts)):
        o["handverts3d"] = v


def _obj_rows(dicts, obj_bank):
    """The dicts' ``obj_info`` rows, checked (all dicts or none, collated, a bank, ids inside it) before anything is uploaded:
    None, or the arguments of ``objgt.obj_geometry_batch``."""
    with_info = sum("obj_info" in d for d in dicts)
    if not with_info:
        return None
    if with_info != len(dicts):
        raise ValueError(f"obj_info in {with_info} of {len(dicts)} dicts: a batch mixes samples of "
                         "HandObjSet(obj_geometry=\"device\") with samples that carry their meshes")
    if obj_bank is None:
        raise ValueError("obj_info needs assemble_batch(obj_bank=...): the bank of the dataset's models")
    from handobjectconsist_amd.datasets import objgt

    rows = [np.asarray(d["obj_info"], np.float32) for d in dicts]
    if any(r.ndim != 2 for r in rows):
        raise ValueError("obj_info must be collated: [frames, values] per dict, not one sample's row")
    args = objgt.unpack_obj_info(np.concatenate(rows, 0))
    obj_bank.check_ids(args["model"])
    return dict(args, groups=[len(r) for r in rows])


def _obj_meshes(args, outs, device, obj_bank):
    """-> ``objverts3d`` / ``objcanverts`` / ``objfaces`` / ``objcantrans`` / ``objcanscale`` in ``outs``, through one
    ``objgt.obj_geometry_batch`` call; each dict padded to its own longest model."""
    from handobjectconsist_amd.datasets import objgt

    for o, res in zip(outs, objgt.obj_geometry_batch(obj_bank, device=device, **args)):
        o.update(res)


def _gt2d_rows(dicts, obj_args, mano_layer):
    """The dicts' ``gt2d_info`` rows, checked (all dicts or none, collated, the rows of the kinds they ask for present) before
    anything is uploaded: None, or the arguments of ``gt2d.points2d_batch`` less the hand's vertices."""
    with_info = sum("gt2d_info" in d for d in dicts)
    if not with_info:
        return None
    if with_info != len(dicts):
        raise ValueError(f"gt2d_info in {with_info} of {len(dicts)} dicts: a batch mixes samples of "
                         "HandObjSet(points2d=\"device\") with samples that carry their 2-D points")
    from handobjectconsist_amd.datasets import gt2d

    rows = [np.asarray(d["gt2d_info"], np.float32) for d in dicts]
    if any(r.ndim != 2 for r in rows):
        raise ValueError("gt2d_info must be collated: [frames, values] per dict, not one sample's row")
    args = gt2d.unpack_gt2d_info(np.concatenate(rows, 0))
    keys = args.pop("keys")
    args.update(groups=[len(r) for r in rows], keys=keys, points2d_mirrored=True)
    if any(k.startswith("objverts2d") for k in keys):
        if obj_args is None:
            raise ValueError("gt2d_info asks for objverts2d: the dicts need obj_info (HandObjSet(obj_geometry=\"device\"))")
        args.update(model=obj_args["model"], pose=obj_args["pose"])
    if any(k.startswith("handverts2d") for k in keys):
        if any("hand_info" not in d for d in dicts) or mano_layer is None:
            raise ValueError("gt2d_info asks for handverts2d: the dicts need hand_info (HandObjSet(hand_geometry=\"device\")) and "
                             "assemble_batch(mano_layer=...)")
    if any(k.startswith("joints2d") for k in keys):
        if any("gt2d_joints" not in d for d in dicts):
            raise ValueError("gt2d_info asks for joints2d: the dicts need gt2d_joints")
        args["points2d"] = np.concatenate([np.asarray(d["gt2d_joints"], np.float32) for d in dicts], 0)
    return args


def _points2d(args, dicts, outs, device, mano_layer, obj_bank):
    """-> the queried ``joints2d`` / ``objverts2d`` / ``handverts2d`` and their ``_trans`` in ``outs``, through one
    ``gt2d.points2d_batch`` call; the hand's camera-frame vertices from one more ``forward_full`` call (``gt2d.hand_cam_verts``)."""
    from handobjectconsist_amd.datasets import gt2d, manogt

    if any(k.startswith("handverts2d") for k in args["keys"]):
        hand = manogt.unpack_hand_info(np.concatenate([np.asarray(d["hand_info"], np.float32) for d in dicts], 0))
        args = dict(args, points3d=gt2d.hand_cam_verts(mano_layer, hand["fullpose"], hand["shape"], hand["trans"], hand["cam_rot"], device=device))
    for o, res in zip(outs, gt2d.points2d_batch(bank=obj_bank if "model" in args else None, device=device, **args)):
        o.update(res)


def _images(dicts, outs, frame_keys, device, inp_res, **to_batch):
    """The dicts' frames (under one of ``frame_keys``: decoded, or packed by one codec) -> ``image`` / ``jittermask`` in
    ``outs``: decode, then ``resize`` where the dicts carry ``resize_to``, then ``color_augment`` where planned, then one ``frames_to_batch(..., **to_batch)``."""
    def packed_codec():
        for codec in framecodec.CODECS:
            n = sum(codec.key in d for d in dicts)
            if n and (n != len(dicts) or any(k in d for d in dicts for k in frame_keys if k != codec.key)):
                raise ValueError(f"{codec.key} in {n} of {len(dicts)} frame dicts: a batch mixes samples of "
                                 "HandObjSet(decode=\"device\") with decoded frames or with frames of another file format")
            if n:
                return codec
        return None

    def resize_target():
        n = sum("resize_to" in d for d in dicts)
        if n and n != len(dicts):
            raise ValueError(f"resize_to in {n} of {len(dicts)} frame dicts: a batch mixes samples of "
                             "HandObjSet(frame_size=...) whose files need a resize with samples whose files do not")
        if not n:
            return None
        sizes = np.concatenate([np.asarray(d["resize_to"]).reshape(-1, 2) for d in dicts], 0)
        if np.any(sizes != sizes[:1]):
            raise ValueError("resize_to: the batch's frames are to be resized to different sizes (one frame size per batch)")
        return int(sizes[0, 0]), int(sizes[0, 1])

    codec = packed_codec()
    resize_to = resize_target()  # (both checks before anything is uploaded)
    key = "frame" if codec is None else codec.key
    rows = [torch.as_tensor(d[key]) for d in dicts]
    if codec is not None:
        if any(r.dim() != 2 for r in rows):
            raise ValueError(f"{key} must be collated: [frames, bytes] per dict, not one sample's flat packed frame")
        if any(r.shape[1] != rows[0].shape[1] for r in rows):
            raise ValueError(f"{key}: the batch's packed frames differ in size (one frame geometry per batch)")
    frames, split = _stack_rows(rows)
    frames = frames.to(device, non_blocking=True) if codec is None else framecodec.decode_packed(codec, frames, device)
    if resize_to is not None:
        frames = frames_mod.resize(frames, resize_to)
    affines = np.concatenate([np.asarray(d["affinetrans"]) for d in dicts], 0)
    flips = np.concatenate([np.asarray(d["flip"]).reshape(-1) for d in dicts], 0)
    planned = sum("color_plan" in d for d in dicts)
    if planned and planned != len(dicts):
        raise ValueError(f"color_plan in {planned} of {len(dicts)} frame dicts: a batch mixes samples of "
                         "HandObjSet(color_fn=\"device\") with samples of a host colour path")
    if planned:
        plans = np.concatenate([np.asarray(d["color_plan"]) for d in dicts], 0)
        frames = frames_mod.color_augment(frames, plans, flip=flips)
    image, mask = frames_mod.frames_to_batch(frames, affines, inp_res, flip=flips, **to_batch)
    for o, im, jm in zip(outs, split(image), split(mask)):
        o["image"], o["jittermask"] = im, jm


def assemble_batch(batch, device, inp_res, normalize_img=False, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                   image_dtype=torch.float32, mask_dtype=torch.float32, mano_layer=None, obj_bank=None):
    """Collated batch (one frame's dict, or a list of them from ``seq_extend_collate``) -> device-resident
    tensors with ``image`` / ``jittermask`` built by the GPU from ``frame`` / ``affinetrans`` / ``flip``.
    All frames of the step go through ONE ``frames_to_batch`` launch -- after ``frames.color_augment`` where the dicts carry
    ``color_plan`` (``HandObjSet(color_fn="device")``).  Dicts with ``frame_jpeg`` instead of ``frame``
    (``HandObjSet(decode="device")``, all of a batch or none): the packed frames are stacked, uploaded in one copy and
    reconstructed by ``jpegdecode.reconstruct`` first; dicts with ``frame_png`` likewise, through ``pngdecode.unfilter``.  A batch
    holds one of the three.  Dicts with ``resize_to`` (``HandObjSet(decode="device", frame_size=...)`` on files of another size, all
    of a batch or none): the decoded frames go through ``frames.resize`` before the colour augmentation.  ``image_dtype`` / ``mask_dtype``: the batch's element
    types as ``frames_to_batch`` takes them (``torch.bfloat16`` / ``torch.uint8``: the compact batch).
    Dicts with ``hand_info`` (``HandObjSet(hand_geometry="device")``, all of a batch or none) need ``mano_layer``, the
    datasets' ``SynthManoLayer``: the rows are stacked and ``manogt.hand_verts_batch`` runs once; its result is each dict's
    ``handverts3d``.
    Dicts with ``obj_info`` (``HandObjSet(obj_geometry="device")``, all of a batch or none) need ``obj_bank``, the
    ``objgt.ObjectBank`` of the dataset's models: one ``objgt.obj_geometry_batch`` call over all frames of the step gives each dict
    its ``objverts3d`` / ``objcanverts`` / ``objfaces`` (int64) / ``objcantrans`` / ``objcanscale``, padded cyclically to the dict's own
    longest model.  A mixed batch, a missing bank and an id outside the bank raise ValueError before anything is uploaded.
    Dicts with ``gt2d_info`` (``HandObjSet(points2d="device")``, all of a batch or none): after the hand and object calls, one
    ``gt2d.points2d_batch`` call over all frames of the step gives each dict the 2-D keys its samples were queried for --
    ``joints2d`` / ``objverts2d`` / ``handverts2d`` and their ``_trans``, float32 [frames, points, 2], ``objverts2d`` padded as
    ``objverts3d`` is.  A dict with 2-D ground truth, from either path, keeps its ``affinetrans`` (the metrics read it)."""
    dicts = batch if isinstance(batch, (list, tuple)) else [batch]
    frame_keys = ("frame",) + tuple(codec.key for codec in framecodec.CODECS)
    consumed = frame_keys + ("affinetrans", "flip", "color_plan", "hand_info", "resize_to", "obj_info", "gt2d_info", "gt2d_joints")
    obj_args = _obj_rows(dicts, obj_bank)  # (refusals before the first upload)
    gt2d_args = _gt2d_rows(dicts, obj_args, mano_layer)
    out = [{k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in d.items() if k not in consumed}
           for d in dicts]
    _hand_verts(dicts, out, device, mano_layer)
    if obj_args is not None:
        _obj_meshes(obj_args, out, device, obj_bank)
    if gt2d_args is not None:
        _points2d(gt2d_args, dicts, out, device, mano_layer, obj_bank)
    for d, o in zip(dicts, out):
        if "affinetrans" in d and ("gt2d_info" in d or any(k in d for k in POINTS2D_KEYS)):
            o["affinetrans"] = torch.as_tensor(d["affinetrans"]).to(device, non_blocking=True)
    with_frames = [i for i, d in enumerate(dicts) if any(k in d for k in frame_keys)]
    if with_frames:
        m, s = (mean, std) if normalize_img else ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0))
        _images([dicts[i] for i in with_frames], [out[i] for i in with_frames], frame_keys, device, inp_res, mean=m,
                std=s, image_dtype=image_dtype, mask_dtype=mask_dtype)
    return out if isinstance(batch, (list, tuple)) else out[0]
