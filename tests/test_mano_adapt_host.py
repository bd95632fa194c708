"""The FPHAB hand-skeleton adaptor without a device: models/manoadapt.ManoAdaptor's torch restatement against the fixture the
reference's own class produced (tests/golden/make_golden_adaptor.py), its constructors and loaders, the argument validation
of mr_mano_adapt_* (before any HIP call), and SynthMeshRegNet's ``mano_fhb_hand`` switch on CPU tensors.

Tolerances: tests/mano_adapt_cases.py's per-element bound, doubled against the fixture (both sides carry fp32 rounding; a
BLAS is free to order a row's 778 products as it likes)."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from tests import mano_adapt_cases as A

CENTERS = (9, 0)


def _adaptor(center, trainable=True):
    from handobjectconsist_amd.models import manoadapt

    ad = manoadapt.ManoAdaptor(None, A.fixture()[f"adaptor_c{center}"])
    ad.adaptor.weight.requires_grad_(trainable)
    return ad


def _bounds(center):
    fx = A.fixture()
    w, v = fx[f"adaptor_c{center}"], fx["verts_m"]
    fwd = A.forward_reference(v, w, center)
    bwd = A.backward_reference(v, w, center, fx["w_verts"], fx["w_joints"])
    raw = A.forward_reference(v, w, -1)
    return fwd, bwd, raw


@pytest.mark.parametrize("center", CENTERS)
def test_the_fixture_meets_the_fp64_formulas(center):
    """the reference's fp32 results lie within the bound of the formulas the kernels are written to: the fixture and the
    header describe the same function"""
    fx = A.fixture()
    fwd, bwd, raw = _bounds(center)
    A.check(f"fixture c{center} adapt_joints", fx[f"c{center}_adapt_joints"], raw["joints_out"])
    A.check(f"fixture c{center} joints3d", fx[f"c{center}_joints3d"], fwd["joints_out"])
    A.check(f"fixture c{center} verts3d", fx[f"c{center}_verts3d"], fwd["verts_out"])
    A.check(f"fixture c{center} grad verts", fx[f"c{center}_grad_verts"], bwd["grad_verts"])
    A.check(f"fixture c{center} grad weight", fx[f"c{center}_grad_weight"], bwd["grad_weight"])


@pytest.mark.parametrize("entry", ["adapt", "forward_torch"])
@pytest.mark.parametrize("center", CENTERS)
def test_cpu_tensors_reproduce_the_fixture(center, entry):
    fx = A.fixture()
    ad = _adaptor(center)
    verts = torch.from_numpy(fx["verts_m"]).clone().requires_grad_(True)
    if entry == "adapt":
        verts_c, joints_c = ad.adapt(verts, center)
        adapt_joints = ad.adapt(verts, None)[1]
    else:  # the reference's four lines (meshregnet.py:193-198) over forward_torch
        out, moved = ad.forward_torch(verts)
        assert tuple(out.shape) == (3, 3, 21) and tuple(moved.shape) == (21, 778) and float(moved.detach().abs().max()) == 0.0
        adapt_joints = out.transpose(1, 2)
        joints_c = adapt_joints - adapt_joints[:, center].unsqueeze(1)
        verts_c = verts - adapt_joints[:, center].unsqueeze(1)
    loss = (torch.from_numpy(fx["w_joints"]) * joints_c).sum() + (torch.from_numpy(fx["w_verts"]) * verts_c).sum()
    g_verts, g_weight = torch.autograd.grad(loss, [verts, ad.adaptor.weight])
    fwd, bwd, raw = _bounds(center)
    for name, got, bound in (("adapt_joints", adapt_joints, raw["joints_out"]), ("joints3d", joints_c, fwd["joints_out"]),
                             ("verts3d", verts_c, fwd["verts_out"]), ("grad_verts", g_verts, bwd["grad_verts"]),
                             ("grad_weight", g_weight, bwd["grad_weight"])):
        ref = fx[f"c{center}_{name}"].astype(np.float64)
        A.check(f"{entry} c{center} {name} against the fixture", got.detach().numpy(), (ref, bound[1]), factor=2.0)


def test_forward_is_the_reference_forward():
    """forward() on CPU tensors: (joints [B,3,21], weight - J_regressor); the wrist and tip rows of a trainable weight are reset
    to the regressor's first, a frozen weight is left as it is"""
    from handobjectconsist_amd.models import manoadapt

    fx = A.fixture()
    verts = torch.from_numpy(fx["verts_m"])
    ad = _adaptor(9)
    with torch.no_grad():
        ad.adaptor.weight.add_(0.25)
    joints, moved = ad(verts)
    assert tuple(joints.shape) == (3, 3, 21)
    rows = list(manoadapt.FIX_IDXS)
    others = [k for k in range(21) if k not in rows]
    assert rows == [0, 4, 8, 12, 16, 20]
    assert torch.equal(ad.adaptor.weight.detach()[rows], ad.J_regressor[rows]) and float(moved.detach()[rows].abs().max()) == 0.0
    assert float((moved.detach()[others] - 0.25).abs().max()) < 1e-6
    raw = A.forward_reference(fx["verts_m"], ad.adaptor.weight.detach().numpy(), -1)["joints_out"]
    A.check("forward, moved weight", joints.detach().transpose(1, 2).numpy(), raw, factor=2.0)
    frozen = _adaptor(9, trainable=False)
    with torch.no_grad():
        frozen.adaptor.weight.add_(0.25)
    frozen(verts)
    assert float((frozen.adaptor.weight - frozen.J_regressor - 0.25).abs().max()) < 1e-6, "a frozen weight is not reset"


def test_constructors_and_loaders(tmp_path):
    from handobjectconsist_amd.models import manoadapt
    from handobjectconsist_amd.models.synthnet import SynthManoLayer

    fx = A.fixture()
    derived = manoadapt.ManoAdaptor(SynthManoLayer())
    assert derived.J_regressor.dtype == torch.float32
    assert np.array_equal(derived.J_regressor.numpy().view(np.uint32), fx["reordered_regressor"].view(np.uint32))
    assert torch.equal(derived.adaptor.weight.detach(), derived.J_regressor)
    assert isinstance(derived.adaptor, torch.nn.Linear) and derived.adaptor.bias is None
    assert (derived.adaptor.in_features, derived.adaptor.out_features) == (778, 21)
    assert sorted(derived.state_dict()) == ["J_regressor", "adaptor.weight"]
    assert "J_regressor" in dict(derived.named_buffers()) and derived.adaptor.weight.requires_grad
    w = fx["adaptor_c9"]
    pkl, npz = tmp_path / "fhb_skel.pkl", tmp_path / "fhb_skel.npz"
    with open(pkl, "wb") as fh:
        pickle.dump({"adaptor": w, "shape": np.zeros(10, np.float32)}, fh)
    np.savez(npz, adaptor=w)
    for source in (str(pkl), str(npz), w, torch.from_numpy(w)):
        ad = manoadapt.ManoAdaptor(None, source)
        assert np.array_equal(ad.J_regressor.numpy().view(np.uint32), w.view(np.uint32))
        assert torch.equal(ad.adaptor.weight.detach(), ad.J_regressor)
        assert ad.adaptor.weight.data_ptr() != ad.J_regressor.data_ptr()
    with pytest.raises(ValueError):
        manoadapt.ManoAdaptor(None, w[:, :700])
    with pytest.raises(ValueError):
        derived(torch.zeros(2, 700, 3))
    with pytest.raises(RuntimeError, match="fp32"):
        manoadapt.adapt_hip(torch.zeros(1, 778, 3), torch.zeros(21, 778), 9)  # (CPU tensors: the kernels are not for them)


def test_argument_validation_needs_no_device():
    """every MR_ERR_BADARG / MR_ERR_NOTIMPL case of the header and B == 0, with made-up non-NULL pointers that are never
    dereferenced: each call returns before the first HIP call"""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    P, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(None)
    assert lib.mr_mano_adapt_workspace_floats(192, 21) == 192 * 21 * 3
    assert lib.mr_mano_adapt_workspace_floats(0, 21) == 0
    assert lib.mr_mano_adapt_workspace_floats(-1, 21) == -1 and lib.mr_mano_adapt_workspace_floats(2, 0) == -1
    assert lib.mr_mano_adapt_workspace_floats(2 ** 31 - 1, 32) == -1  # (the count is an int)
    assert lib.mr_mano_adapt_workspace_floats(22369621, 32) == 22369621 * 96 and lib.mr_mano_adapt_workspace_floats(22369622, 32) == -1

    def fwd(verts=P, weight=P, center=9, verts_out=P, joints_out=P, B=2, V=778, J=21):
        return lib.mr_mano_adapt_forward(verts, weight, center, verts_out, joints_out, B, V, J, None)

    def bwd(verts=P, weight=P, center=9, g_verts=P, g_joints=P, work=P, grad_verts=P, grad_weight=P, B=2, V=778, J=21):
        return lib.mr_mano_adapt_backward(verts, weight, center, g_verts, g_joints, work, grad_verts, grad_weight, B, V, J, None)

    for call in (fwd, bwd):
        assert call(B=0) == 0
        assert call(B=0, center=-1, V=1, J=1) == 0
        for bad in (dict(B=-1), dict(V=0), dict(V=-5), dict(J=0), dict(center=-2), dict(center=21), dict(center=1, J=1),
                    dict(B=0, center=21), dict(B=0, V=0), dict(verts=null), dict(weight=null),
                    dict(verts=ctypes.c_void_p(0x1002))):
            assert call(**bad) == -1, (call.__name__, bad)
        for big in (dict(J=33), dict(V=4097), dict(J=33, center=32), dict(J=64, V=8192)):
            assert call(**big) == -2, (call.__name__, big)
        assert call(B=0, J=33) == 0
    assert fwd(verts_out=null) == -1 and fwd(joints_out=null) == -1
    assert bwd(work=null) == -1 and bwd(grad_verts=null) == -1
    # absent incoming gradients and an absent weight gradient are arguments like any other: the limits are still seen
    assert bwd(g_verts=null, g_joints=null, grad_weight=null, J=33) == -2
    assert bwd(g_verts=null, g_joints=null, grad_weight=null, center=30) == -1
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.call("mr_mano_adapt_forward", P, P, 21, P, P, 2, 778, 21, None)
    with pytest.raises(RuntimeError, match="not implemented"):
        _lib.call("mr_mano_adapt_backward", P, P, 0, P, P, P, P, null, 2, 4097, 21, None)
    assert _lib.call("mr_mano_adapt_forward", P, P, 9, P, P, 0, 778, 21, None) == 0


def test_default_network_is_what_it_was():
    from handobjectconsist_amd.models import synthnet

    plain, off = synthnet.SynthMeshRegNet(), synthnet.SynthMeshRegNet(mano_fhb_hand=False)
    assert off.adaptor is None and not off.mano_fhb_hand
    assert list(plain.state_dict()) == list(off.state_dict())
    assert {k.split(".")[0] for k in off.state_dict()} == {"base_net", "scaletrans_branch", "scaletrans_branch_obj", "mano_base", "pose_reg",
                                                          "shape_reg", "mano_layer"}
    on = synthnet.SynthMeshRegNet(mano_fhb_hand=True)
    assert sorted(set(on.state_dict()) - set(off.state_dict())) == ["adaptor.J_regressor", "adaptor.adaptor.weight"]
    assert set(off.state_dict()) <= set(on.state_dict())
    assert not any(p.requires_grad for p in on.adaptor.parameters()), "the adaptor is frozen (rec_freeze)"
    assert np.array_equal(on.adaptor.J_regressor.numpy(), A.fixture()["reordered_regressor"])
    trainable = lambda m: [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable(on) == trainable(off)


def test_network_on_cpu_post_processes_the_fixture_joints():
    """SynthMeshRegNet(mano_fhb_hand=True).post_heads on CPU tensors: recov_joints3d = recover_3d_proj of the fixture's centred
    joints, recov_handverts3d = the fixture's centred vertices + the recovered centre.  The network adapts millimetres and
    divides by 1000 afterwards where the fixture adapted metres: the bound of the adapted values (doubled, both sides round)
    plus four units in the last place of the result for the division and the centre's addition on either side."""
    from handobjectconsist_amd.models import synthnet

    fx = A.fixture()
    net = synthnet.SynthMeshRegNet(mano_fhb_hand=True, fhb_adaptor=fx["adaptor_c9"]).eval()
    B = 3
    g = torch.Generator().manual_seed(4)
    scaletrans, st_obj = torch.randn(B, 3, generator=g), torch.randn(B, 6, generator=g)
    camintr = torch.tensor([[350.0, 0.0, 120.0], [0.0, 350.0, 131.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    canverts = 0.05 * torch.randn(B, 30, 3, generator=g)
    pose, betas = torch.from_numpy(fx["pose"]), torch.from_numpy(fx["betas"])
    with torch.no_grad():
        handverts3d, joints3d, joints2d, objverts3d, objverts2d = net.post_heads(pose, betas, scaletrans, st_obj, camintr, canverts)
        want_joints, center3d = synthnet.recover_3d_proj(torch.from_numpy(fx["c9_joints3d"]), camintr,
                                                         scaletrans[:, :1].view(-1, 1, 1) * net.obj_scale_factor,
                                                         scaletrans[:, 1:].unsqueeze(1) * net.obj_trans_factor, input_res=(256, 256))
        want_verts = torch.from_numpy(fx["c9_verts3d"]) + center3d
    assert tuple(joints3d.shape) == (B, 21, 3) and tuple(joints2d.shape) == (B, 21, 2) and tuple(handverts3d.shape) == (B, 778, 3)
    fwd = A.forward_reference(fx["verts_m"], fx["adaptor_c9"], 9)
    for name, got, want, bound in (("recov_joints3d", joints3d, want_joints, fwd["joints_out"][1]),
                                   ("recov_handverts3d", handverts3d, want_verts, fwd["verts_out"][1])):
        want = want.numpy().astype(np.float64)
        A.check(f"network on CPU: {name}", got.numpy(), (want, 2 * bound + 4 * A.ulp32(want)))
    # ... and it is not what the network without the switch computes
    plain = synthnet.SynthMeshRegNet().eval()
    with torch.no_grad():
        other = plain.post_heads(pose, betas, scaletrans, st_obj, camintr, canverts)[1]
    assert float((other - joints3d).abs().max()) > 1e-3
