"""The general MANO call and the ground-truth hand meshes, host side: ``hand_verts_host`` and ``forward_full`` on
CPU tensors against oracle/mano_ref.py, the untouched default of ``SynthPoseDataset``, and the new C-ABI symbols' argument
validation without a device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mano_ref as M

BUFFERS = ("th_v_template", "th_shapedirs", "th_posedirs", "th_J_regressor", "th_weights", "th_comps", "th_hands_mean")


def consts(layer):
    return {k: getattr(layer, k).detach().cpu().numpy() for k in BUFFERS}


def within(got, ref, what):
    """the tolerance of tests/test_gpu_warp.py::test_mano_lbs_hip_matches_the_numpy_oracle: 1e-5 (1 + max |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, tol = float(np.abs(got - ref).max()), 1e-5 * (1.0 + float(np.abs(ref).max()))
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def gt_reference(c, fullpose, shape, trans, cam_rot, flip, rot_mat, center3d):
    """The oracle per sample in fp64, then the reference's numpy lines."""
    out = []
    for i in range(len(fullpose)):
        verts, _ = M.mano_forward(c, fullpose[i:i + 1], shape[i:i + 1], use_pca=False, center_idx=None)
        verts = verts[0] / 1000 + trans[i]                                   # fhbhands.py:358, ho3dv2.py:346
        if cam_rot is not None:
            verts = cam_rot.dot(verts.transpose()).transpose()               # ho3dv2.py:347
        pts = np.array(verts)                                                # handobjset.py:160-164
        if flip[i]:
            pts[:, 0] = -pts[:, 0]
        pts = rot_mat[i].dot(pts.transpose(1, 0)).transpose()                # handobjset.py:166-167, 181
        out.append(pts - center3d[i] if center3d is not None else pts)       # handobjset.py:182
    return np.stack(out)


def gt_inputs(n, seed):
    rng = np.random.default_rng(seed)
    fullpose = np.concatenate([rng.standard_normal((n, 3)) * 0.8, rng.standard_normal((n, 45)) * 0.3], 1).astype(np.float32)
    shape = rng.standard_normal((n, 10)).astype(np.float32)
    trans = (rng.standard_normal((n, 3)) * 0.2 + [0, 0, 0.6]).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, n)
    rot_mat = np.stack([np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) for a in ang]).astype(np.float32)
    flip = np.arange(n) % 2 == 1
    cam_rot = M.batch_rodrigues(np.array([[0.3, -1.1, 0.4]]))[0].astype(np.float32)  # (float32: a packed row holds it exactly)
    center3d = (rng.standard_normal((n, 3)) * 0.1 + [0, 0, 0.6]).astype(np.float32)
    return fullpose, shape, trans, cam_rot, flip, rot_mat, center3d


@pytest.mark.parametrize("with_cam,with_center", [(False, True), (True, False), (True, True)])
def test_hand_verts_host_matches_the_oracle(with_cam, with_center):
    from handobjectconsist_amd.datasets import manogt
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    fullpose, shape, trans, cam_rot, flip, rot_mat, center3d = gt_inputs(5, 3)
    cam_rot, center3d = cam_rot if with_cam else None, center3d if with_center else None
    got = manogt.hand_verts_host(layer, fullpose, shape, trans, cam_rot=cam_rot, flip=flip, rot_mat=rot_mat, center3d=center3d)
    assert got.dtype == np.float32 and got.shape == (5, 778, 3)
    within(got, gt_reference(consts(layer), fullpose, shape, trans, cam_rot, flip, rot_mat, center3d), "hand_verts_host")
    # ... and the packed row HandObjSet hands to assemble_batch is the same call
    rows = np.stack([manogt.pack_hand_info(fullpose[i], trans[i], shape[i], flip[i], rot_mat[i],
                                           None if center3d is None else center3d[i], cam_rot) for i in range(5)])
    again = manogt.hand_verts_host(layer, **manogt.unpack_hand_info(rows))
    assert np.array_equal(again, got)
    with pytest.raises(ValueError, match="some rows carry"):
        rows[0, 71] = 1 - rows[0, 71]
        manogt.unpack_hand_info(rows)


VARIANTS = [dict(use_pca=False, flat_hand_mean=True, center_idx=None, trans=False),
            dict(use_pca=False, flat_hand_mean=False, center_idx=9, trans=False),
            dict(use_pca=True, flat_hand_mean=False, center_idx=8, trans=False),
            dict(use_pca=True, flat_hand_mean=False, center_idx=9, trans=True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"pca{int(v['use_pca'])}-c{v['center_idx']}-t{int(v['trans'])}")
def test_forward_full_on_cpu_tensors_matches_the_oracle(variant):
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(ncomps=15, use_pca=variant["use_pca"], flat_hand_mean=variant["flat_hand_mean"],
                                    center_idx=variant["center_idx"])
    g = torch.Generator().manual_seed(11)
    B = 3
    pose = 0.4 * torch.randn(B, 18 if variant["use_pca"] else 48, generator=g)
    pose[0, :3] = 0
    beta = torch.randn(B, 10, generator=g)
    trans = 0.1 * torch.randn(B, 3, generator=g) if variant["trans"] else None
    kw = dict(use_pca=variant["use_pca"], center_idx=variant["center_idx"], trans=None if trans is None else trans.numpy())
    v, j = layer.forward_full(pose, beta, trans)
    v_ref, j_ref = M.mano_forward(consts(layer), pose.numpy(), beta.numpy(), **kw)
    within(v.numpy(), v_ref, "verts")
    within(j.numpy(), j_ref, "joints")
    # manopth's rule: an all-zero translation counts as absent
    v0, j0 = layer.forward_full(pose, beta, torch.zeros(B, 3))
    vn, jn = layer.forward_full(pose, beta, None)
    assert torch.equal(v0, vn) and torch.equal(j0, jn)
    # the epilogue, restated in torch, against the same lines in numpy on the oracle's output
    rng = np.random.default_rng(5)
    rot = M.batch_rodrigues(rng.standard_normal((B, 3)))
    t1, t2 = rng.standard_normal((B, 3)) * 0.3, rng.standard_normal((B, 3)) * 0.3
    vp, jp = layer.forward_full(pose, beta, trans, post={"scale": 1e-3, "trans": t1, "rot": rot, "trans2": t2})
    ref = np.einsum("bij,bvj->bvi", rot, v_ref * 1e-3 + t1[:, None]) - t2[:, None]
    within(vp.numpy(), ref, "verts after the epilogue")
    within(jp.numpy(), np.einsum("bij,bvj->bvi", rot, j_ref * 1e-3 + t1[:, None]) - t2[:, None], "joints after the epilogue")
    assert not vp.requires_grad and not jp.requires_grad and jp.shape == (B, 21, 3)
    with pytest.raises(ValueError, match="pose must be"):
        layer.forward_full(torch.zeros(B, 20), beta)
    with pytest.raises(ValueError, match="center_idx"):
        synthnet.SynthManoLayer(use_pca=False, center_idx=21).forward_full(torch.zeros(B, 48), beta)


def test_synth_pose_dataset_without_a_layer_is_unchanged():
    """Values recorded from the parent commit for seed 3 (num_pairs=2, frame_size=(96, 64))."""
    from handobjectconsist_amd.datasets.synthpose import SynthPoseDataset

    ds = SynthPoseDataset(num_pairs=2, frame_size=(96, 64), seed=3)
    assert ds.mano_infos is None
    with pytest.raises(RuntimeError, match="no MANO annotations"):
        ds.get_hand_info(0)
    f = lambda a: np.asarray(a, np.float64).reshape(-1).tolist()
    got = {"frames_sum": int(ds.frames.astype(np.int64).sum()), "frame0": ds.frames[0, 0, :2].tolist(),
           "hand1": f(ds.get_hand_verts3d(1)[[0, 777]]), "joints2": f(ds.get_joints3d(2)[0]), "obj3": f(ds.get_obj_verts_trans(3)[0]),
           "K0": f(ds.get_camintr(0)), "center_scale": f(ds.get_center_scale(1)[0]) + [ds.get_center_scale(1)[1]],
           "can": f(ds.can_trans) + [ds.can_scale]}
    assert got["frames_sum"] == RECORDED["frames_sum"] and got["frame0"] == RECORDED["frame0"]  # (integers: exact)
    for key in ("hand1", "joints2", "obj3", "K0", "center_scale", "can"):
        # (float32 values of the seeded scene; 1e-6 relative: one ulp of room for another host's libm, nothing a change hides in)
        assert np.allclose(got[key], RECORDED[key], rtol=1e-6, atol=0), key


RECORDED = {'frames_sum': 9406241,
 'frame0': [[248, 194, 190], [207, 147, 26]],
 'hand1': [0.004630775656551123,
           -0.008121425285935402,
           0.415976345539093,
           -0.01019249763339758,
           -0.043309979140758514,
           0.4299832582473755],
 'joints2': [-0.016071362420916557, 0.03608220815658569, 0.4120703637599945],
 'obj3': [0.031076163053512573, -0.013783987611532211, 0.48168429732322693],
 'K0': [308.5649108886719, 0.0, 52.82038879394531, 0.0, 308.5649108886719, 33.31459045410156, 0.0, 0.0, 1.0],
 'center_scale': [74.59285736083984, 4.75462532043457, 182.76116943359375],
 'can': [0.031998805701732635, -0.017859434708952904, 0.43593379855155945, 0.08438097685575485]}


def test_synth_pose_dataset_with_a_layer_serves_mano_meshes():
    from handobjectconsist_amd.datasets.synthpose import SynthPoseDataset
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    ds, plain = SynthPoseDataset(num_pairs=2, frame_size=(96, 64), seed=3, mano_layer=layer), SynthPoseDataset(num_pairs=2, frame_size=(96, 64), seed=3)
    assert np.array_equal(ds.frames, plain.frames) and np.array_equal(ds.get_joints3d(1), plain.get_joints3d(1))
    pose, trans, shape = ds.get_hand_info(2)
    assert pose.shape == (48,) and trans.shape == (3,) and shape.shape == (10,)
    v_ref, _ = M.mano_forward(consts(layer), pose[None], shape[None], use_pca=False, center_idx=None)
    within(ds.get_hand_verts3d(2), v_ref[0] / 1000 + trans, "get_hand_verts3d")
    with pytest.raises(ValueError, match="use_pca=False"):
        SynthPoseDataset(num_pairs=1, mano_layer=synthnet.SynthManoLayer(use_pca=True))


def test_hand_geometry_device_refusals_need_no_device():
    from handobjectconsist_amd.datasets import handobjset, manogt
    from handobjectconsist_amd.datasets.synthpose import SynthPoseDataset

    class NoInfo:
        def __len__(self):
            return 1

    with pytest.raises(ValueError, match="get_hand_info"):
        handobjset.HandObjSet(NoInfo(), hand_geometry="device")
    with pytest.raises(ValueError, match="hand_geometry must be"):
        handobjset.HandObjSet(SynthPoseDataset(num_pairs=1, frame_size=(96, 64)), hand_geometry="gpu")
    with pytest.raises(ValueError, match="hand_cam_rot"):  # (the host path calls get_hand_verts3d itself: nothing would use it)
        handobjset.HandObjSet(SynthPoseDataset(num_pairs=1, frame_size=(96, 64)), hand_cam_rot=np.eye(3))
    row = np.zeros((2, manogt.HAND_INFO_FLOATS), np.float32)
    with pytest.raises(ValueError, match="mixes samples"):
        handobjset.assemble_batch([{"hand_info": row}, {"handverts3d": torch.zeros(2, 778, 3)}], "cpu", (64, 64))
    with pytest.raises(ValueError, match="mano_layer"):
        handobjset.assemble_batch([{"hand_info": row}], "cpu", (64, 64))


def test_the_camera_rotation_of_the_device_path_is_stated_never_read_from_the_dataset():
    """fhbhands.py:75-82 defines ``cam_extr`` and its ``get_hand_verts3d`` (:355-359) does not apply it; ho3dv2.py:347 does.  An
    attribute cannot tell the two apart, so the packed row carries a rotation only where ``hand_cam_rot`` states one."""
    from handobjectconsist_amd.datasets import handobjset, manogt
    from handobjectconsist_amd.datasets.synthpose import SynthPoseDataset
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    ds = SynthPoseDataset(num_pairs=1, frame_size=(96, 64), seed=3, mano_layer=layer)
    ds.cam_extr = np.eye(4)
    ds.cam_extr[:3, :3] = M.batch_rodrigues(np.array([[0.003, -0.004, 0.001]]))[0]  # (about 0.005 rad, as FHB's)
    cam_rot = ds.cam_extr[:3, :3].astype(np.float32)
    kw = dict(inp_res=(64, 64), hand_geometry="device", color_fn=None)
    row = handobjset.HandObjSet(ds, **kw)[0]["hand_info"]
    info = manogt.unpack_hand_info(row[None])
    assert info["cam_rot"] is None and np.array_equal(info["fullpose"][0], ds.get_hand_info(0)[0])
    row = handobjset.HandObjSet(ds, hand_cam_rot=ds.cam_extr[:3, :3], **kw)[0]["hand_info"]
    assert np.array_equal(manogt.unpack_hand_info(row[None])["cam_rot"][0], cam_rot)
    with pytest.raises(ValueError, match="3x3"):
        handobjset.HandObjSet(ds, hand_cam_rot=ds.cam_extr, **kw)


def test_full_entry_points_validate_before_any_device_work():
    """B == 0 is MR_OK; NULL or misaligned pointers, ncomps outside 1..45, a centre outside -1..20 and an unknown pose form
    are MR_ERR_BADARG -- all without a device (no HIP call happens before the checks)."""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    assert lib.mr_mano_full_workspace_floats(-1) == -1
    assert lib.mr_mano_full_workspace_floats(0) == 0
    assert lib.mr_mano_full_workspace_floats(33) == lib.mr_mano_workspace_floats(33) + 33
    null, p = ctypes.c_void_p(None), ctypes.c_void_p(4096)   # (never dereferenced: every call below returns before a launch)
    odd = ctypes.c_void_p(4098)

    def fwd(B=1, form=0, ncomps=15, center=9, pose=p, comps=p, trans=null, post_trans=null, post_rot=null, work=p, verts=p):
        return lib.mr_mano_forward_full(pose, p, trans, comps, p, p, p, p, p, p, p, p, p, form, ncomps, center, 1.0, post_trans,
                                        post_rot, null, work, verts, p, B, null)

    def bwd(B=1, form=0, ncomps=15, center=9, comps=p, g_pose=p, g_trans=null):
        return lib.mr_mano_backward_full(comps, p, p, p, p, p, p, p, p, p, form, ncomps, center, p, null, null, g_pose, p, g_trans,
                                         B, null)

    assert fwd(B=0, pose=null, comps=null, work=null) == 0 and bwd(B=0, comps=null, g_pose=null) == 0
    assert fwd(B=-1) == -1 and bwd(B=-1) == -1 and fwd(B=65536) == -1 and bwd(B=65536) == -1
    for bad in (dict(form=2), dict(form=-1), dict(ncomps=0), dict(ncomps=46), dict(center=-2), dict(center=21), dict(comps=null),
                dict(comps=odd)):
        assert fwd(**bad) == -1, bad
        assert bwd(**bad) == -1, bad
    for bad in (dict(pose=null), dict(pose=odd), dict(work=null), dict(verts=null), dict(verts=odd), dict(trans=odd),
                dict(post_trans=p), dict(post_rot=odd)):
        assert fwd(**bad) == -1, bad
    assert bwd(g_pose=null) == -1 and bwd(g_pose=odd) == -1 and bwd(g_trans=odd) == -1
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.call("mr_mano_forward_full", *([null] * 13), 1, 45, 20, 1.0, *([null] * 6), 1, null)
