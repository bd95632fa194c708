"""mr_mano_forward_full / mr_mano_backward_full against oracle/mano_ref.py -- manopth's ManoLayer.forward restated
joint by joint in numpy, OUTSIDE the product: the full axis-angle pose, a finger-tip centre, a translation under manopth's
all-zero rule, the ground-truth epilogue (``manogt.hand_verts_batch``) and the dataset path that uses it.  Tolerances: those
of tests/test_gpu_warp.py::test_mano_lbs_hip_matches_the_numpy_oracle -- values within 1e-5 (1 + max |ref|), directional
derivatives within 1e-4 max(|num|, 1) + 1e-4 max |grad|."""
import random

import numpy as np
import pytest
import torch

from oracle import mano_ref as M

pytestmark = pytest.mark.gpu
BUFFERS = ("th_v_template", "th_shapedirs", "th_posedirs", "th_J_regressor", "th_weights", "th_comps", "th_hands_mean")


def consts(layer):
    return {k: getattr(layer, k).detach().cpu().numpy() for k in BUFFERS}


def within(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, tol = float(np.abs(got - ref).max()), 1e-5 * (1.0 + float(np.abs(ref).max()))
    print(f"{what}: max err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


# (use_pca, flat_hand_mean, center_idx, translation): the datasets' layer; an articulated centre on the axis-angle form; the
# three tip centres the reorder table puts at 4, 8 and 20; manobranch's call with th_trans
VARIANTS = [(False, True, None, False), (False, False, 9, False), (True, False, 4, False), (True, False, 8, False),
            (True, False, 20, False), (True, False, 9, True)]


@pytest.mark.parametrize("B", [1, 33, 2])
@pytest.mark.parametrize("use_pca,flat,center_idx,with_trans", VARIANTS)
def test_forward_full_matches_the_numpy_oracle(cuda, use_pca, flat, center_idx, with_trans, B):
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(ncomps=15, use_pca=use_pca, flat_hand_mean=flat, center_idx=center_idx).to(cuda)
    c = consts(layer)
    g = torch.Generator().manual_seed(300 + B)
    pose = 0.4 * torch.randn(B, 18 if use_pca else 48, generator=g)
    pose[0, :3] = 0  # a zero axis-angle: the 1e-8 guard of the Rodrigues formula
    beta = torch.randn(B, 10, generator=g)
    trans = 0.1 * torch.randn(B, 3, generator=g) if with_trans else None
    kw = dict(use_pca=use_pca, center_idx=center_idx)
    p, b_ = pose.to(cuda).requires_grad_(True), beta.to(cuda).requires_grad_(True)
    t_ = trans.to(cuda).requires_grad_(True) if with_trans else None
    v_hip, j_hip = layer.forward_full(p, b_, t_)
    v_ref, j_ref = M.mano_forward(c, pose.numpy(), beta.numpy(), trans=None if trans is None else trans.numpy(), **kw)
    within(v_hip.detach().cpu().numpy(), v_ref, "verts")
    within(j_hip.detach().cpu().numpy(), j_ref, "joints")
    wv, wj = torch.randn(v_hip.shape, generator=g), torch.randn(j_hip.shape, generator=g)
    ((v_hip * wv.to(cuda)).sum() + (j_hip * wj.to(cuda)).sum()).backward()
    gp, gb = p.grad.double().cpu(), b_.grad.double().cpu()
    gt = t_.grad.double().cpu() if with_trans else None
    assert gp.shape == pose.shape and gb.shape == beta.shape

    def loss_of_trans(tt):
        v, j = M.mano_forward(c, pose.numpy(), beta.numpy(), trans=tt, dtype=np.float64, **kw)
        return float((v * wv.numpy()).sum() + (j * wj.numpy()).sum())

    for k in range(4):
        dp, db = torch.randn(pose.shape, generator=g), torch.randn(beta.shape, generator=g)
        if k == 0:
            dp[1:], db[1:] = 0, 0  # sample 0 alone (its root rotation is the guarded zero axis-angle)
        num = M.directional_derivative(c, pose.numpy(), beta.numpy(), wv.numpy(), wj.numpy(), dp.numpy(), db.numpy(),
                                       trans=None if trans is None else trans.numpy().astype(np.float64), **kw)
        ana = float((gp * dp.double()).sum() + (gb * db.double()).sum())
        if with_trans:  # the translation's direction: a second difference quotient, the oracle untouched
            dt, eps, t64 = torch.randn(B, 3, generator=g).double().numpy(), 1e-6, trans.double().numpy()
            num += (loss_of_trans(t64 + eps * dt) - loss_of_trans(t64 - eps * dt)) / (2 * eps)
            ana += float((gt.numpy() * dt).sum())
        bound = 1e-4 * max(abs(num), 1.0) + 1e-4 * float(gp.abs().max())
        print(f"direction {k}: analytic {ana:.9e}, numeric {num:.9e}, |diff| {abs(ana - num):.3e}, bound {bound:.3e}")
        assert abs(ana - num) <= bound, (k, ana, num)


@pytest.mark.parametrize("center_idx", [9, 8])
def test_all_zero_translation_counts_as_absent(cuda, center_idx):
    """manopth's rule on the device: zeros (of either sign) give the centred result, bit for bit that of trans=None; ONE
    sample with a non-zero translation leaves every sample uncentred."""
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(ncomps=15, use_pca=True, center_idx=center_idx).to(cuda)
    c, B = consts(layer), 5
    g = torch.Generator().manual_seed(7)
    pose, beta = 0.4 * torch.randn(B, 18, generator=g), torch.randn(B, 10, generator=g)
    p, b_ = pose.to(cuda), beta.to(cuda)
    v_none, j_none = layer.forward_full(p, b_, None)
    zeros = torch.zeros(B, 3)
    zeros[2, 1] = -0.0
    tz = zeros.to(cuda).requires_grad_(True)
    v_zero, j_zero = layer.forward_full(p, b_, tz)
    assert torch.equal(v_zero.detach(), v_none) and torch.equal(j_zero.detach(), j_none)
    (v_zero.sum() + j_zero.sum()).backward()
    assert torch.equal(tz.grad, torch.zeros_like(tz))  # an absent translation has no gradient
    v_ref, j_ref = M.mano_forward(c, pose.numpy(), beta.numpy(), trans=zeros.numpy(), center_idx=center_idx)
    within(v_zero.detach().cpu().numpy(), v_ref, "verts, zero translation")
    within(j_zero.detach().cpu().numpy(), j_ref, "joints, zero translation")
    one = torch.zeros(B, 3)
    one[3, 2] = 0.25
    v_one, j_one = layer.forward_full(p, b_, one.to(cuda))
    v_ref, j_ref = M.mano_forward(c, pose.numpy(), beta.numpy(), trans=one.numpy(), center_idx=center_idx)
    within(v_one.cpu().numpy(), v_ref, "verts, one sample translated")
    within(j_one.cpu().numpy(), j_ref, "joints, one sample translated")
    assert float((v_one[0] - v_none[0]).abs().max()) > 1.0  # sample 0, itself untranslated, is no longer centred (millimetres)


@pytest.mark.parametrize("B", [2, 33])
def test_forward_full_equals_forward_where_both_apply(cuda, B):
    """PCA coefficients, centre 9, no translation, no epilogue: the same bits, values and gradients (the shared kernels are the
    same templates, the adjoint order is kept)."""
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(ncomps=15, use_pca=True, center_idx=9).to(cuda)
    g = torch.Generator().manual_seed(B)
    pose, beta = 0.4 * torch.randn(B, 18, generator=g), torch.randn(B, 10, generator=g)
    wv, wj = torch.randn(B, 778, 3, generator=g).to(cuda), torch.randn(B, 21, 3, generator=g).to(cuda)
    grads = []
    for fn in (layer.forward, layer.forward_full):
        p, b_ = pose.to(cuda).requires_grad_(True), beta.to(cuda).requires_grad_(True)
        v, j = fn(p, b_)
        ((v * wv).sum() + (j * wj).sum()).backward()
        grads.append((v.detach(), j.detach(), p.grad, b_.grad))
    for a, b, what in zip(grads[0], grads[1], ("verts", "joints", "grad pose", "grad betas")):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("use_pca,center_idx,with_trans,on_device", [(True, 9, True, True), (True, 8, False, False),
                                                                      (False, None, False, True)],
                         ids=["centre9-translated", "tip-centre", "axisang-uncentred"])
def test_forward_full_epilogue_on_verts_and_joints(cuda, use_pca, center_idx, with_trans, on_device):
    """``post`` through ``forward_full`` itself: the 778 vertices, the 16 joint rows and the 5 tip rows against the oracle
    followed by x = rot (v scale + trans) - trans2 in fp64 -- with a ``th_trans`` in force, with a tip centre (subtracted
    after the skin, before the epilogue) and on the datasets' form; ``post`` as CUDA tensors and as host arrays."""
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(ncomps=15, use_pca=use_pca, flat_hand_mean=not use_pca, center_idx=center_idx).to(cuda)
    B, g, rng = 3, torch.Generator().manual_seed(17), np.random.default_rng(17)
    pose, beta = 0.4 * torch.randn(B, 18 if use_pca else 48, generator=g), torch.randn(B, 10, generator=g)
    trans = 0.1 * torch.randn(B, 3, generator=g) if with_trans else None
    rot = M.batch_rodrigues(rng.standard_normal((B, 3))).astype(np.float32)
    t1, t2 = (rng.standard_normal((B, 3)) * 0.3).astype(np.float32), (rng.standard_normal((B, 3)) * 0.3).astype(np.float32)
    post = {"scale": 1e-3, "trans": t1, "rot": rot, "trans2": t2}
    if on_device:
        post = {k: (torch.from_numpy(a).to(cuda) if isinstance(a, np.ndarray) else a) for k, a in post.items()}
    p = pose.to(cuda).requires_grad_(True)
    v, j = layer.forward_full(p, beta.to(cuda), None if trans is None else trans.to(cuda), post=post)
    assert v.shape == (B, 778, 3) and j.shape == (B, 21, 3) and not v.requires_grad and not j.requires_grad
    v_ref, j_ref = M.mano_forward(consts(layer), pose.numpy(), beta.numpy(), trans=None if trans is None else trans.numpy(),
                                  use_pca=use_pca, center_idx=center_idx)
    epilogue = lambda x: np.einsum("bij,bvj->bvi", rot.astype(np.float64), x * 1e-3 + t1[:, None]) - t2[:, None]
    within(v.cpu().numpy(), epilogue(v_ref), "verts after the epilogue")
    within(j.cpu().numpy(), epilogue(j_ref), "joints after the epilogue")


def gt_reference(c, fullpose, shape, trans, cam_rot, flip, rot_mat, center3d):
    """The oracle per sample in fp64, then the reference's numpy lines."""
    out = []
    for i in range(len(fullpose)):
        verts, _ = M.mano_forward(c, fullpose[i:i + 1], shape[i:i + 1], use_pca=False, center_idx=None)
        verts = verts[0] / 1000 + trans[i]                                   # fhbhands.py:358, ho3dv2.py:346
        if cam_rot is not None:
            verts = cam_rot.dot(verts.transpose()).transpose()               # ho3dv2.py:347
        pts = np.array(verts)                                                # handobjset.py:160-164 (mirrored)
        if flip[i]:
            pts[:, 0] = -pts[:, 0]
        pts = rot_mat[i].dot(pts.transpose(1, 0)).transpose()                # handobjset.py:166-167, 181 (rotated)
        out.append(pts - center3d[i] if center3d is not None else pts)       # handobjset.py:182
    return np.stack(out)


@pytest.mark.parametrize("with_cam,with_center", [(False, True), (True, False), (True, True)])
def test_hand_verts_batch_matches_the_oracle_and_the_host_path(cuda, with_cam, with_center):
    from handobjectconsist_amd.datasets import manogt
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)  # (on the CPU: the datasets' own)
    n, rng = 5, np.random.default_rng(3)
    fullpose = np.concatenate([rng.standard_normal((n, 3)) * 0.8, rng.standard_normal((n, 45)) * 0.3], 1).astype(np.float32)
    shape = rng.standard_normal((n, 10)).astype(np.float32)
    trans = (rng.standard_normal((n, 3)) * 0.2 + [0, 0, 0.6]).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, n)
    rot_mat = np.stack([np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) for a in ang]).astype(np.float32)
    rot_mat[4] = np.eye(3)
    flip = np.arange(n) % 2 == 1
    cam_rot = M.batch_rodrigues(np.array([[0.3, -1.1, 0.4]]))[0] if with_cam else None
    center3d = (rng.standard_normal((n, 3)) * 0.1 + [0, 0, 0.6]).astype(np.float32) if with_center else None
    kw = dict(cam_rot=cam_rot, flip=flip, rot_mat=rot_mat, center3d=center3d)
    got = manogt.hand_verts_batch(layer, fullpose, shape, trans, device=cuda, **kw)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (n, 778, 3) and not got.requires_grad
    within(got.cpu().numpy(), gt_reference(consts(layer), fullpose, shape, trans, cam_rot, flip, rot_mat, center3d), "hand_verts_batch")
    within(got.cpu().numpy(), manogt.hand_verts_host(layer, fullpose, shape, trans, **kw), "hand_verts_batch vs hand_verts_host")


@pytest.mark.parametrize("opt_ins", [dict(color_fn=None), dict(color_fn="device", decode="device")],
                         ids=["geometry-alone", "with-decode-and-colour"])
def test_hand_geometry_device_equals_host_through_the_dataset(cuda, opt_ins):
    """Same seeds -> same draws, RNG streams at the same position, the same images and masks bit for bit, and the hand
    vertices of the GPU call within the tolerance of the host path's."""
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.models import synthnet
    from handobjectconsist_amd.utils import collate

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    out, states = {}, {}
    for geometry in ("host", "device"):
        ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=(272, 248), seed=1, sides=("right", "left"), mano_layer=layer,
                                        jpeg_quality=90 if opt_ins.get("decode") == "device" else None)
        hs = handobjset.HandObjSet(ds, inp_res=(64, 64), sample_nb=2, sides="right", hand_geometry=geometry, **opt_ins)
        random.seed(21)
        np.random.seed(21)
        torch.manual_seed(21)
        batch = collate.seq_extend_collate([hs[i] for i in (0, 3)], ["objverts3d", "objfaces", "objcanverts"])
        states[geometry] = (random.getstate(), np.random.get_state()[1].tolist(), torch.get_rng_state())
        out[geometry] = handobjset.assemble_batch(batch, cuda, (64, 64), mano_layer=layer)
        if geometry == "device":
            assert all("handverts3d" not in d and d["hand_info"].shape == (2, 85) for d in batch)
    assert states["host"][0] == states["device"][0] and states["host"][1] == states["device"][1]
    assert torch.equal(states["host"][2], states["device"][2])
    for fa, fb in zip(out["host"], out["device"]):
        assert fa.keys() == fb.keys() and "hand_info" not in fb
        assert torch.equal(fa["image"], fb["image"]) and torch.equal(fa["jittermask"], fb["jittermask"])
        assert torch.equal(fa["joints3d"], fb["joints3d"]) and torch.equal(fa["objverts3d"], fb["objverts3d"])
        assert fb["handverts3d"].is_cuda and fb["handverts3d"].shape == (2, 778, 3)
        within(fb["handverts3d"].cpu().numpy(), fa["handverts3d"].cpu().numpy(), "handverts3d, device vs host")


@pytest.mark.parametrize("applies_cam_extr", [True, False], ids=["ho3d-style", "fhb-style"])
def test_hand_geometry_device_with_a_dataset_that_has_cam_extr(cuda, applies_cam_extr):
    """Both of the reference's datasets define ``cam_extr``.  ho3dv2.py:346-347 rotates the hand vertices by it, and
    ``hand_cam_rot`` says so; fhbhands.py:355-359 does not (its ``cam_extr``, :75-82, serves the skeleton and the object), and
    the device path must not apply it either.  Either way device equals host."""
    from handobjectconsist_amd.datasets import handobjset, manogt, synthpose
    from handobjectconsist_amd.models import synthnet
    from handobjectconsist_amd.utils import collate

    class CamDataset(synthpose.SynthPoseDataset):
        cam_extr = np.eye(4)
        cam_extr[:3, :3] = M.batch_rodrigues(np.array([[0.3, -1.1, 0.4]]))[0]

        def get_hand_verts3d(self, idx):
            pose, trans, shape = self.get_hand_info(idx)
            cam_rot = self.cam_extr[:3, :3] if applies_cam_extr else None
            return manogt.hand_verts_host(self.mano_layer, pose[None], shape[None], trans[None], cam_rot=cam_rot)[0]

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    ds = CamDataset(num_pairs=2, frame_size=(272, 248), seed=2, sides=("right", "left"), mano_layer=layer)
    out = {}
    for geometry in ("host", "device"):
        kw = dict(hand_cam_rot=ds.cam_extr[:3, :3]) if applies_cam_extr and geometry == "device" else {}
        hs = handobjset.HandObjSet(ds, inp_res=(64, 64), sides="right", color_fn=None, hand_geometry=geometry, **kw)
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(5)
        batch = collate.extend_collate([hs[i] for i in (0, 1, 2)], ["objverts3d", "objfaces", "objcanverts"])
        out[geometry] = handobjset.assemble_batch(batch, cuda, (64, 64), mano_layer=layer)["handverts3d"]
    assert out["device"].is_cuda and out["device"].shape == (3, 778, 3)
    within(out["device"].cpu().numpy(), out["host"].cpu().numpy(), "handverts3d, device vs host")
    # the yardstick outside the product, for frame 1 (a left hand: mirrored): the oracle and the reference's numpy lines
    pose, trans, shape = ds.get_hand_info(1)
    ref = gt_reference(consts(layer), pose[None], shape[None], trans[None], ds.cam_extr[:3, :3] if applies_cam_extr else None,
                       [False], [np.eye(3)], None)[0]
    within(ds.get_hand_verts3d(1), ref, "get_hand_verts3d of the dataset")


def test_hand_verts_batch_follows_weights_loaded_after_the_first_call(cuda):
    """The device copy of a CPU layer is keyed on the layer's buffers: ``load_state_dict`` of other MANO weights after a first
    call must not leave the GPU serving the meshes of the old ones."""
    from handobjectconsist_amd.datasets import manogt
    from handobjectconsist_amd.models import synthnet

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    rng = np.random.default_rng(9)
    fullpose, shape = (rng.standard_normal((2, 48)) * 0.3).astype(np.float32), rng.standard_normal((2, 10)).astype(np.float32)
    trans = np.zeros((2, 3), np.float32)
    first = manogt.hand_verts_batch(layer, fullpose, shape, trans, device=cuda)
    layer.load_state_dict(synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None, seed=1).state_dict())
    second = manogt.hand_verts_batch(layer, fullpose, shape, trans, device=cuda)
    ref = gt_reference(consts(layer), fullpose, shape, trans, None, [False, False], [np.eye(3)] * 2, None)
    within(second.cpu().numpy(), ref, "hand_verts_batch after load_state_dict")
    assert float((second - first).abs().max()) > 1e-4  # (the two seeds' hands differ by far more than the tolerance, in metres)


def test_refusals_launch_nothing(cuda):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import handobjset, manogt
    from handobjectconsist_amd.models import synthnet

    calls = []
    real_call = _lib.call

    def counting_call(name, *args):
        calls.append(name)
        return real_call(name, *args)

    _lib.call = counting_call
    try:
        pca = synthnet.SynthManoLayer(ncomps=15, use_pca=True, center_idx=9).to(cuda)
        axis = synthnet.SynthManoLayer(ncomps=15, use_pca=False, center_idx=None).to(cuda)
        pose, beta = torch.zeros(2, 18, device=cuda), torch.zeros(2, 10, device=cuda)
        with pytest.raises(RuntimeError, match="fp32"):
            pca.forward_full(pose.double(), beta.double())
        with pytest.raises(RuntimeError, match="fp32"):
            pca.forward_full(pose, beta.double())
        with pytest.raises(ValueError, match="pose must be"):
            pca.forward_full(torch.zeros(2, 48, device=cuda), beta)
        with pytest.raises(ValueError, match="pose must be"):
            axis.forward_full(pose, beta)
        with pytest.raises(ValueError, match="center_idx"):
            synthnet.SynthManoLayer(ncomps=15, use_pca=True, center_idx=21).to(cuda).forward_full(pose, beta)
        with pytest.raises(RuntimeError, match="buffers are on cpu"):  # (a layer left on the host: refused, no host pointer launched)
            synthnet.SynthManoLayer(ncomps=15, use_pca=True, center_idx=9).forward_full(pose, beta)
        row = np.zeros((2, manogt.HAND_INFO_FLOATS), np.float32)
        with pytest.raises(ValueError, match="mixes samples"):
            handobjset.assemble_batch([{"hand_info": row}, {"handverts3d": torch.zeros(2, 778, 3)}], cuda, (64, 64), mano_layer=axis)
        with pytest.raises(ValueError, match="get_hand_info"):
            handobjset.HandObjSet(object(), hand_geometry="device")
        # ... and SynthManoLayer.forward keeps its three refusals
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            pca(pose, beta, th_trans=torch.ones(2, 3, device=cuda))
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            pca(pose.double(), beta.double())
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            axis(torch.zeros(2, 48, device=cuda), beta)
    finally:
        _lib.call = real_call
    assert calls == []
