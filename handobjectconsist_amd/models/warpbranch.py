"""Photometric-consistency branch: meshes of a frame sequence -> rendered optical flows -> pair
losses.  Counterpart of meshreg/models/warpbranch.py:9-96 (same ``forward`` argument list and
return value) organised as three steps:

1. ``_frame_meshes``  hand + object vertices per frame; with ``gt_refs`` every frame after the
   first is replaced by its ground-truth geometry (warpbranch.py:38-47); frames after the first
   are constants for autograd when ``first_only`` (:53-54); hand and object are concatenated into
   one mesh with offset face indices (:49-55).
2. ``get_opticalflows`` with the reference's training setting ``detach_textures=False,
   detach_renders=True`` (:59-68): gradients reach the vertices only through the flow VALUES.
3. one ``pair_consist`` per (frame 0, frame k) pair, averaged (:73-88).

Samples are dicts of tensors keyed like the reference's (``TransQueries.IMAGE / JITTERMASK / CAMINTR``,
``BaseQueries.OBJFACES`` and, for annotated frames, ``BaseQueries.HANDVERTS3D / OBJVERTS3D``:
datasets/queries.py) or by the plain strings "image", "jittermask", "camintr", "objfaces",
"handverts3d", "objverts3d" the synthetic loaders of this package use."""
import torch

from handobjectconsist_amd.datasets.queries import lookup as _q
from handobjectconsist_amd.warping import imgflowarp, opticalflow


_FACES_CACHE = {}


def _cat_faces(hand_face, obj_faces, batch, hand_verts):
    """Faces of the concatenated hand + object mesh (object indices offset by the hand's vertex count).
    Index tensors that are the same objects step after step (a fixed object model, the synthetic
    loader's pool) give the same result tensor back, which also keeps the renderer's own face cache warm."""
    key = tuple((x.data_ptr(), x._version, tuple(x.shape), x.dtype, str(x.device)) for x in (hand_face, obj_faces)) \
        + (batch, hand_verts)
    hit = _FACES_CACHE.get("last")
    if hit is None or hit[0] != key:
        hand_faces = hand_face.long().unsqueeze(0) if hand_face.dim() == 2 else hand_face.long()
        if hand_faces.shape[0] == 1:  # warpbranch.py:36: hand_face.repeat(batch, 1, 1)
            hand_faces = hand_faces.expand(batch, -1, -1)
        faces = torch.cat([hand_faces, obj_faces.long().cuda() + hand_verts], 1)
        hit = (key, faces, hand_face, obj_faces)  # holds the inputs: their addresses stay unique while cached
        _FACES_CACHE["last"] = hit
    return hit[1]


def _frame_meshes(samples, all_results, hand_face, gt_refs, first_only):
    batch = all_results[0]["recov_objverts3d"].shape[0]
    frames = []
    for k, (sample, result) in enumerate(zip(samples, all_results)):
        annotated = gt_refs and k > 0
        hand = _q(sample, "handverts3d").cuda() if annotated else result["recov_handverts3d"]
        obj = _q(sample, "objverts3d").cuda() if annotated else result["recov_objverts3d"]
        verts = torch.cat([hand, obj], 1)
        frames.append(verts.detach() if (first_only and k > 0) else verts)
    # the reference concatenates the faces of every frame and keeps the LAST frame's (warpbranch.py:49-55)
    faces = _cat_faces(hand_face, _q(samples[-1], "objfaces"), batch, hand.shape[1])
    return frames, faces


def _frame_parts(samples, all_results, gt_refs, first_only):
    """(hand, object) vertices per frame as ``_frame_meshes`` selects them, NOT concatenated."""
    frames = []
    for k, (sample, result) in enumerate(zip(samples, all_results)):
        annotated = gt_refs and k > 0
        hand = _q(sample, "handverts3d").cuda() if annotated else result["recov_handverts3d"]
        obj = _q(sample, "objverts3d").cuda() if annotated else result["recov_objverts3d"]
        frames.append((hand.detach(), obj.detach()) if (first_only and k > 0) else (hand, obj))
    return frames


def _fused_pairs(samples, all_results, hand_face, gt_refs, first_only, renderer, image_size, hand_ignore_faces, use_backward,
                 crit):
    """The "loss" mode of ``forward`` with every (frame 0, frame k) pair as ONE fused node (opticalflow.flow_pair_loss:
    render, then occlusion + epilogue + pair loss in one pass, one backward launch; hand and object go in as separate
    tensors, concatenated by index inside the kernels); None when the node does not apply.  ``crit``: MR_CRITERION_* of the
    pair loss (imgflowarp._fused_criterion)."""
    cams = [_q(sample, "camintr").cuda() for sample in samples]
    ref_image, ref_jitter = _q(samples[0], "image").cuda(), _q(samples[0], "jittermask").cuda()
    parts = _frame_parts(samples, all_results, gt_refs, first_only)
    faces = (hand_face.cuda(), _q(samples[-1], "objfaces").cuda())  # (the LAST frame's faces, warpbranch.py:49-55)
    losses, flows, means = [], [], []
    for k in range(1, len(samples)):
        res = opticalflow.flow_pair_loss([parts[0], parts[k]], faces, [cams[0], cams[k]], renderer, image_size,
                                         ref_image, _q(samples[k], "image").cuda(), ref_jitter,
                                         _q(samples[k], "jittermask").cuda(), ignore_face_idxs=hand_ignore_faces, with_sum=True,
                                         with_mean="sum" if use_backward else "fwd", criterion=crit)
        if res is None:
            return None if k == 1 else _raise_mixed()
        loss_fwd, loss_bwd, pair_flows, loss_sum, mean = res
        losses.append(loss_sum if use_backward else loss_fwd)  # (loss_sum = loss_bwd + loss_fwd, formed by the node itself)
        flows.append(pair_flows)
        means.append(mean)
    # (one pair -- the trainer's setting --: the stack is a view, not a copy launch, and the mean over the batch is the
    # node's own output: warpbranch.py:87-88's stack(...).mean() without a reduction launch and its backward)
    diff_losses = losses[0].unsqueeze(0) if len(losses) == 1 else torch.stack(losses)
    none = [None] * len(losses)
    return (means[0] if len(means) == 1 else diff_losses.mean()), {"masks": none, "warps": list(none), "recons_flows": flows,
                                                                  "diffs": list(none), "diff_losses": diff_losses}


def _raise_mixed():
    raise RuntimeError("the fused pair node applied to the first frame pair of a sequence but not to a later one")


def forward(
    samples,
    all_results,
    hand_face,
    renderer,
    image_size,
    criterion,
    gt_refs=True,
    first_only=True,
    hand_ignore_faces=None,
    use_backward=True,
    pair_outputs="full",
):
    """
    Args:
        samples / all_results: per-frame inputs and network outputs; frame 0 is the frame under
            supervision-by-consistency, later frames are the references it is compared with
        hand_face: closed hand faces [F,3] (or already batched [B,F,3])
        use_backward: also compare the warp of the unannotated frame with the annotated image
        pair_outputs: "full" (masks / warps / diffs as the reference returns them) or "loss" (the trainer's setting:
            masks / warps / diffs are None and ``recons_flows`` hold defined values only where their renders cover
            something -- ``flow._base._hoc_coverage`` -- everything else is unspecified memory;
            ``opticalflow.dense_flows(pair_flows)`` returns zero-filled copies for logging or visualisation)

    Returns:
        (mean pair loss, {"masks", "warps", "recons_flows", "diffs", "diff_losses"})
    """
    crit = imgflowarp._fused_criterion(criterion)  # (l1 / l2: the fused pair kernels; None: anything else)
    if pair_outputs == "loss" and crit is not None:
        fused = _fused_pairs(samples, all_results, hand_face, gt_refs, first_only, renderer, image_size, hand_ignore_faces,
                             use_backward, crit)
        if fused is not None:
            return fused
    verts_world, all_faces = _frame_meshes(samples, all_results, hand_face, gt_refs, first_only)
    recons_flows = opticalflow.get_opticalflows(
        verts_world,
        all_faces,
        [_q(sample, "camintr").cuda() for sample in samples],
        renderer,
        image_size,
        detach_textures=False,
        detach_renders=True,
        ignore_face_idxs=hand_ignore_faces,
        # "loss": nobody but pair_consist looks at the flows -- they (and the gradient that comes back for them) are then
        # computed and stored under the renders' covered tiles only.  Only where pair_consist reads them with the fused
        # kernels (a criterion they compute): the composed path samples the flows over the whole image.
        sparse_flows=(pair_outputs == "loss" and crit is not None),
    )
    ref_image, ref_jitter = _q(samples[0], "image").cuda(), _q(samples[0], "jittermask").cuda()
    per_pair = [
        imgflowarp.pair_consist(
            flow,
            image_ref=ref_image,
            image=_q(sample, "image").cuda(),
            jitter_mask_ref=ref_jitter,
            jitter_mask=_q(sample, "jittermask").cuda(),
            criterion=criterion,
            use_backward=use_backward,
            outputs=pair_outputs,
        )
        for flow, sample in zip(recons_flows, samples[1:])
    ]
    diff_losses = torch.stack([res[0] for res in per_pair])
    pair_results = {
        "masks": [res[1] for res in per_pair],
        "warps": [res[2] for res in per_pair],
        "recons_flows": recons_flows,
        "diffs": [res[3] for res in per_pair],
        "diff_losses": diff_losses,
    }
    return diff_losses.mean(), pair_results
