"""mr_mano_adapt_forward / _backward (csrc/mano_adapt.hip) and the layers above them on a device: MeshRegNet's FPHAB
hand-skeleton adaptor.

Values: every output and gradient, element by element, against the fp64 numpy evaluation of the header's formulas under
tests/mano_adapt_cases.py's bound (2 n 2^-24 sum |terms| + 2 ulp; nothing is taken from a run), at the shapes that cross
every boundary of the kernels -- a wave is 64 lanes, a workgroup 256: partial waves, one lane, more joints than waves, the
LDS limit -- and, doubled, against the fixture the reference's own class produced.  Output buffers are pre-filled with NaN:
an element nobody writes fails the finiteness check.

Also: two calls give the same bits; a sample's results do not depend on its batch; either incoming gradient absent; the
weight gradient asked for or not (then never allocated, and no second launch's pointer); guard bands intact; strided inputs
through the Python layer; the call on a side stream behind a delay (tests/test_gpu_side_stream.py's arrangement) and under
one hipGraph capture replayed twice on changed inputs (tests/test_gpu_graph_replay.py's recipe), since the host recorder
does not link this source; the network with ``mano_fhb_hand=True`` against its own op-by-op branch; the refusals.

Measured on an MI355X (``MANO-ADAPT ...`` lines), largest error / bound: vertices 0.13 and joints 0.07 (at the few-term shapes
(2, 1, 1, 0) and (2, 5, 3, 2); 0.001 at V = 778), vertex gradients 0.15 (without a centre; 0.004 with one), gt 0.04, weight
gradient 0.23; against the fixture 0.005 of the doubled bound.  Side stream: largest |side - default| 0 over all four outputs
behind a 19.97 ms delay.  The whole file takes 5 s.
"""
import numpy as np
import pytest
import torch

from tests import mano_adapt_cases as A

pytestmark = pytest.mark.gpu


def up(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)  # (a copy: the cases' arrays are read-only)


def bits(t):
    return t.detach().contiguous().view(torch.uint8)


def run_raw(cuda, verts, weight, center, g_verts, g_joints, want_weight=True):
    """the three entry points as they are, on NaN-filled outputs -> dict of device tensors"""
    from handobjectconsist_amd import _lib

    P = _lib.ptr
    v, w, gv, gj = (up(a, cuda) for a in (verts, weight, g_verts, g_joints))
    (B, V, _), J = v.shape, w.shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)
    out = dict(verts_out=nan(B, V, 3), joints_out=nan(B, J, 3), grad_verts=nan(B, V, 3), grad_weight=nan(J, V) if want_weight else None)
    floats = _lib.load().mr_mano_adapt_workspace_floats(B, J)
    assert floats == B * J * 3
    out["gt"] = nan(B, J, 3)
    _lib.call("mr_mano_adapt_forward", P(v), P(w), center, P(out["verts_out"]), P(out["joints_out"]), B, V, J, _lib.stream_ptr(cuda))
    _lib.call("mr_mano_adapt_backward", P(v), P(w), center, P(gv), P(gj), P(out["gt"]), P(out["grad_verts"]), P(out["grad_weight"]),
              B, V, J, _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    return out


def check_all(what, got, verts, weight, center, g_verts, g_joints, factor=1.0):
    ref = dict(A.forward_reference(verts, weight, center), **A.backward_reference(verts, weight, center, g_verts, g_joints))
    for name, value in got.items():
        if value is not None:
            A.check(f"{what} {name}", value.cpu().numpy(), ref[name], factor)


# ---- values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=str)
def test_values_against_fp64(cuda, shape):
    """forward, vertex gradient, gt and weight gradient with both incoming gradients present; a second call has the same bits"""
    verts, weight, g_verts, g_joints = A.inputs(shape)
    center = shape[3]
    got = run_raw(cuda, verts, weight, center, g_verts, g_joints)
    check_all(str(shape), got, verts, weight, center, g_verts, g_joints)
    again = run_raw(cuda, verts, weight, center, g_verts, g_joints)
    for name in got:
        assert torch.equal(bits(got[name]), bits(again[name])), f"{shape} {name}: two calls differ"
    if center >= 0:
        assert float(got["joints_out"][:, center].abs().max()) == 0.0, "the centre joint is the origin"
    else:
        assert torch.equal(bits(got["verts_out"]), bits(up(verts, cuda))), "no centre: the vertices as they came"


@pytest.mark.parametrize("shape", [(3, 778, 21, 9), (2, 65, 21, 9), (2, 257, 2, -1)], ids=str)
@pytest.mark.parametrize("absent", ["g_joints", "g_verts", "grad_weight"])
def test_absent_gradients(cuda, shape, absent):
    """g_joints or g_verts NULL means zeros: values against the formulas with zeros, and the same bits as a call that passes
    zeros; grad_weight NULL: the vertex gradient and gt have the bits of the call that asked for it"""
    verts, weight, g_verts, g_joints = A.inputs(shape)
    center = shape[3]
    if absent == "grad_weight":
        got = run_raw(cuda, verts, weight, center, g_verts, g_joints, want_weight=False)
        full = run_raw(cuda, verts, weight, center, g_verts, g_joints)
        assert got["grad_weight"] is None
        check_all(f"{shape} without grad_weight", got, verts, weight, center, g_verts, g_joints)
    else:
        gv, gj = (None, g_joints) if absent == "g_verts" else (g_verts, None)
        got = run_raw(cuda, verts, weight, center, gv, gj)
        check_all(f"{shape} without {absent}", got, verts, weight, center, gv, gj)
        full = run_raw(cuda, verts, weight, center, np.zeros_like(g_verts) if gv is None else gv, np.zeros_like(g_joints) if gj is None else gj)
    for name in ("grad_verts", "gt") + (() if absent == "grad_weight" else ("grad_weight",)):
        assert torch.equal(bits(got[name]), bits(full[name])), f"{shape} without {absent}: {name}"


@pytest.mark.parametrize("shape", [(3, 778, 21, 0), (3, 778, 21, 20), (3, 65, 21, 9)], ids=str)
def test_a_sample_does_not_depend_on_its_batch(cuda, shape):
    verts, weight, g_verts, g_joints = A.inputs(shape)
    center = shape[3]
    batch = run_raw(cuda, verts, weight, center, g_verts, g_joints)
    alone = run_raw(cuda, verts[1:2], weight, center, g_verts[1:2], g_joints[1:2])
    for name in ("verts_out", "joints_out", "grad_verts", "gt"):
        assert torch.equal(bits(batch[name][1:2]), bits(alone[name])), f"{shape}: {name} of sample 1 alone differs"
    # (the weight gradient sums over the batch; alone it is the one sample's term)
    A.check(f"{shape} sample 1 alone grad_weight", alone["grad_weight"].cpu().numpy(),
            A.backward_reference(verts[1:2], weight, center, g_verts[1:2], g_joints[1:2])["grad_weight"])


@pytest.mark.parametrize("center", [9, 0])
def test_kernels_against_the_reference_run_fixture(cuda, center):
    """the reference's own ManoAdaptor on the CPU (metres): the bound, doubled -- both sides carry rounding"""
    from handobjectconsist_amd.models import manoadapt

    fx = A.fixture()
    verts, weight = fx["verts_m"], fx[f"adaptor_c{center}"]
    got = run_raw(cuda, verts, weight, center, fx["w_verts"], fx["w_joints"])
    fwd, bwd = A.forward_reference(verts, weight, center), A.backward_reference(verts, weight, center, fx["w_verts"], fx["w_joints"])
    for name, key, bound in (("joints_out", "joints3d", fwd["joints_out"]), ("verts_out", "verts3d", fwd["verts_out"]),
                             ("grad_verts", "grad_verts", bwd["grad_verts"]), ("grad_weight", "grad_weight", bwd["grad_weight"])):
        A.check(f"fixture c{center} {key}", got[name].cpu().numpy(), (fx[f"c{center}_{key}"].astype(np.float64), bound[1]), factor=2.0)
    # the module's forward(): joints [B,3,21] as a transposed view, and what the weight has moved by
    ad = manoadapt.ManoAdaptor(None, weight).to(cuda)
    joints, moved = ad(up(verts, cuda))
    assert tuple(joints.shape) == (3, 3, 21) and joints.stride() == (63, 1, 3) and float(moved.detach().abs().max()) == 0.0
    raw = A.forward_reference(verts, weight, -1)["joints_out"]
    A.check(f"fixture c{center} adapt_joints", joints.detach().transpose(1, 2).cpu().numpy(),
            (fx[f"c{center}_adapt_joints"].astype(np.float64), raw[1]), factor=2.0)
    v_c, j_c = ad.adapt(up(verts, cuda), center)
    assert torch.equal(bits(v_c), bits(got["verts_out"])) and torch.equal(bits(j_c), bits(got["joints_out"]))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def layer_run(verts, weight, center, g_verts, g_joints, weight_grad=True):
    """adapt_hip + autograd.grad on device tensors -> [verts_out, joints_out, grad verts, grad weight | None]"""
    from handobjectconsist_amd.models import manoadapt

    v = verts.detach().requires_grad_(True)
    w = weight.detach().requires_grad_(weight_grad)
    vo, jo = manoadapt.adapt_hip(v, w, center)
    outs, gouts = [o for o, g in ((vo, g_verts), (jo, g_joints)) if g is not None], [g for g in (g_verts, g_joints) if g is not None]
    grads = torch.autograd.grad(outs, [v, w] if weight_grad else [v], gouts)
    return [vo.detach(), jo.detach(), grads[0], grads[1] if weight_grad else None]


NAMES = ["verts_out", "joints_out", "grad_verts", "grad_weight"]


@pytest.mark.parametrize("weight_grad", [True, False], ids=["weight-gradient", "frozen-weight"])
def test_autograd_function(cuda, monkeypatch, weight_grad):
    """the Function gives the raw calls' bits; a weight gradient is requested only when needs_input_grad says so: otherwise the
    entry point gets NULL and nothing of the weight's shape is allocated"""
    from handobjectconsist_amd import _lib

    shape = (3, 778, 21, 9)
    verts, weight, g_verts, g_joints = A.inputs(shape)
    raw = run_raw(cuda, verts, weight, 9, g_verts, g_joints)
    calls, made = [], []
    real_call, real_like = _lib.call, torch.empty_like
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append((n, a)), real_call(n, *a))[1])
    monkeypatch.setattr(torch, "empty_like", lambda t, *a, **kw: (made.append(tuple(t.shape)), real_like(t, *a, **kw))[1])
    got = layer_run(up(verts, cuda), up(weight, cuda), 9, up(g_verts, cuda), up(g_joints, cuda), weight_grad)
    monkeypatch.undo()
    assert [n for n, _ in calls] == ["mr_mano_adapt_forward", "mr_mano_adapt_backward"]
    grad_weight_arg = calls[1][1][7]
    assert (grad_weight_arg is not None) == weight_grad
    assert ((21, 778) in made) == weight_grad, made
    for name, g in zip(NAMES, got):
        if g is not None:
            assert torch.equal(bits(g), bits(raw[name])), name
    # one incoming gradient only: autograd hands the Function None for the other, the entry point NULL
    for gv, gj in ((None, g_joints), (g_verts, None)):
        part = layer_run(up(verts, cuda), up(weight, cuda), 9, up(gv, cuda), up(gj, cuda), weight_grad)
        want = run_raw(cuda, verts, weight, 9, gv, gj, weight_grad)
        for name, g in zip(NAMES[2:], part[2:]):
            if g is not None:
                assert torch.equal(bits(g), bits(want[name])), (name, gv is None)


def test_strided_inputs_are_made_dense(cuda):
    """a transposed and an offset-view input through the Python layer: the same bits as the dense tensors"""
    shape = (3, 778, 21, 9)
    verts, weight, g_verts, g_joints = (up(a, cuda) for a in A.inputs(shape))
    want = layer_run(verts, weight, 9, g_verts, g_joints)
    transposed = verts.transpose(0, 1).contiguous().transpose(0, 1)       # [B,V,3] over [V,B,3] memory
    inner = torch.full((5, 780, 3), float("nan"), device=cuda)
    inner[1:4, 1:779] = verts
    offset_verts = inner[1:4, 1:779]                                      # storage offset, rows of 780
    wide = torch.full((23, 778), float("nan"), device=cuda)
    wide[1:22] = weight
    offset_weight = wide[1:22]                                            # dense behind a storage offset
    g_t = g_joints.transpose(1, 2).contiguous().transpose(1, 2)
    assert not transposed.is_contiguous() and not offset_verts.is_contiguous() and offset_weight.storage_offset() == 778
    for what, v, w, gj in (("transposed", transposed, weight, g_t), ("offset views", offset_verts, offset_weight, g_joints)):
        got = layer_run(v, w, 9, g_verts, gj)
        for name, a, b in zip(NAMES, got, want):
            assert torch.equal(bits(a), bits(b)), f"{what}: {name}"


@pytest.mark.parametrize("shape", [(3, 778, 21, 9), (2, 65, 21, 9)], ids=str)
def test_guard_bands(cuda, monkeypatch, shape):
    """forward and backward (weight gradient included) with every tensor inside guard bands: no band changes, every pointer
    the entry points get lies inside a guarded interior, and the values are those of the plain run"""
    from handobjectconsist_amd import _lib
    from tests import guarded_alloc as G

    center = shape[3]
    real = [up(a, cuda) for a in A.inputs(shape)]
    plain = layer_run(real[0], real[1], center, real[2], real[3])
    torch.cuda.synchronize()
    alloc = G.GuardedAllocator(cuda)
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append((n, a)), real_call(n, *a))[1])
    alloc.install(monkeypatch)
    try:
        guarded_in = [alloc.guard(t) for t in real]
        got = layer_run(guarded_in[0], guarded_in[1], center, guarded_in[2], guarded_in[3])
        damage = alloc.check()
    finally:
        alloc.uninstall()
        monkeypatch.setattr(_lib, "call", real_call)
    strangers = alloc.pointer_report(calls)
    print(f"MANO-ADAPT guard bands {shape}: {alloc.count()} guarded allocations, {alloc.pointers_seen} pointer arguments")
    assert not damage, "\n".join(damage)
    assert not strangers, strangers
    assert [n for n, _ in calls] == ["mr_mano_adapt_forward", "mr_mano_adapt_backward"] and alloc.pointers_seen == 4 + 7
    for name, a, b in zip(NAMES, got, plain):
        assert alloc.holds(a), f"{name}: not in guarded storage"
        assert torch.equal(bits(a), bits(b)), name


# ---- streams -------------------------------------------------------------------------------------------------------------------
from tests.test_gpu_side_stream import delay  # noqa: E402,F401  (the session's calibrated delay, as that file measures it)


def test_side_stream_behind_a_delay(cuda, delay):  # noqa: F811
    """forward + backward through the Python layer on a side stream whose inputs arrive after a 20 ms delay kernel: a launch on
    any other stream would read the stale NaN buffers.  Every output has the default stream's bits."""
    from tests import test_gpu_side_stream as SS

    shape = (3, 778, 21, 9)
    real = [up(a, cuda) for a in A.inputs(shape)]
    side = SS.run_family(delay, f"mano adaptor {shape}", real, lambda v, w, gv, gj: layer_run(v, w, 9, gv, gj), NAMES, [SS.EXACT] * 4)
    verts, weight, g_verts, g_joints = A.inputs(shape)
    check_all(f"side stream {shape}", dict(zip(NAMES, side)), verts, weight, 9, g_verts, g_joints)


def test_graph_replay(cuda):
    """one capture of forward + backward (with the weight gradient's second launch), replayed twice on changed inputs: the
    eager default-stream call's bits each time"""
    from tests.test_gpu_graph_replay import capture

    sets = [[up(a, cuda) for a in A.inputs(s)] for s in ((3, 778, 21, 9), (3, 778, 21, 20), (3, 778, 21, 0))]
    assert not torch.equal(sets[0][0], sets[1][0]) and not torch.equal(sets[1][1], sets[2][1])
    eager = [layer_run(*s[:2], 9, *s[2:]) for s in sets]
    torch.cuda.synchronize()
    static = [t.clone() for t in sets[0]]
    graph, side, out = capture(lambda: layer_run(static[0], static[1], 9, static[2], static[3]))
    torch.cuda.synchronize()
    for k in (1, 2):
        for t, r in zip(static, sets[k]):
            t.copy_(r)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(NAMES, out, eager[k]):
            assert torch.equal(bits(a), bits(b)), f"replay {k}: {name} differs from the eager call on the same inputs"
        assert not torch.equal(bits(out[1]), bits(eager[0][1])), "the replay ran on the refreshed inputs"


# ---- the network -----------------------------------------------------------------------------------------------------------------
def test_network_matches_its_op_by_op_branch(cuda, monkeypatch):
    """SynthMeshRegNet(mano_fhb_hand=True).post_heads at B = 2: MANO -> mr_mano_adapt_* -> mr_meshreg_post_* against the same
    network with USE_HIP_POST off (the adaptor through forward_torch, the post-processing op by op); all five results and the
    gradients of the heads' outputs under tests/test_gpu_warp.py's rule for post_heads"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.models import synthnet
    from tests.test_gpu_warp import close

    B, Vo = 2, 130
    model = synthnet.SynthMeshRegNet(mano_fhb_hand=True, fhb_adaptor=A.fixture()["adaptor_c9"]).to(cuda).eval()
    g = torch.Generator().manual_seed(7)
    mk = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g)).to(cuda)
    pose, shape, st, so = mk(B, 18, s=0.3), mk(B, 10), mk(B, 3), mk(B, 6)
    K = torch.tensor([[350.0, 0.0, 120.0], [0.0, 350.0, 131.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).to(cuda)
    can = mk(B, Vo, 3, s=0.05)
    outs, seen = {}, {}
    real_call = _lib.call
    for hip in (True, False):
        calls = seen[hip] = []
        monkeypatch.setattr(_lib, "call", lambda n, *a, _calls=calls: (_calls.append(n), real_call(n, *a))[1])
        monkeypatch.setattr(synthnet, "USE_HIP_POST", hip)
        leaves = [t_.clone().requires_grad_(True) for t_ in (pose, shape, st, so)]
        o = model.post_heads(*leaves, K, can, input_res=(256, 240))
        ws = [torch.randn(x.shape, generator=torch.Generator().manual_seed(k)).to(cuda) for k, x in enumerate(o)]
        sum((a * w).sum() for a, w in zip(o, ws)).backward()
        outs[hip] = (o, leaves)
    monkeypatch.setattr(_lib, "call", real_call)
    assert [n for n in seen[True] if "adapt" in n] == ["mr_mano_adapt_forward", "mr_mano_adapt_backward"]
    assert not [n for n in seen[False] if "adapt" in n or "post" in n]
    for a, b_, name in zip(outs[True][0], outs[False][0], ("handverts3d", "joints3d", "joints2d", "objverts3d", "objverts2d")):
        close(a.detach().cpu().numpy(), b_.detach().cpu().numpy(), 1e-5, 1e-5 * float(b_.detach().abs().max()), name)
    for a, b_, name in zip(outs[True][1], outs[False][1], ("pose", "shape", "scaletrans", "st_obj")):
        assert a.grad is not None and float(a.grad.abs().max()) > 0
        close(a.grad.cpu().numpy(), b_.grad.cpu().numpy(), 2e-4, 2e-5 * float(b_.grad.abs().max()) + 1e-12, f"grad {name}")
    assert model.adaptor.adaptor.weight.grad is None, "the adaptor is frozen"
    plain = synthnet.SynthMeshRegNet().to(cuda).eval()
    with torch.no_grad():
        other = plain.post_heads(pose, shape, st, so, K, can, input_res=(256, 240))[1]
    assert float((other - outs[True][0][1]).abs().max()) > 1e-3, "the switch changes the joints"


# ---- the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda):
    from handobjectconsist_amd.models import manoadapt

    w = A.fixture()["adaptor_c9"]
    on_gpu, on_cpu = manoadapt.ManoAdaptor(None, w).to(cuda), manoadapt.ManoAdaptor(None, w)
    verts = up(A.fixture()["verts_m"], cuda)
    for call in (on_gpu, lambda v: on_gpu.adapt(v, 9)):
        with pytest.raises(RuntimeError, match="fp32"):
            call(verts.to(torch.bfloat16))
        with pytest.raises(RuntimeError, match="fp32"):
            call(verts.double())
    for call in (on_cpu, lambda v: on_cpu.adapt(v, 9)):
        with pytest.raises(RuntimeError, match="move the layer"):
            call(verts)
    with pytest.raises(RuntimeError, match="move the layer"):
        on_gpu(verts.cpu())
    with pytest.raises(RuntimeError, match="fp32"):
        manoadapt.adapt_hip(verts.to(torch.bfloat16), up(w, cuda), 9)
    with pytest.raises(RuntimeError, match="not implemented"):
        manoadapt.adapt_hip(torch.zeros(1, 4097, 3, device=cuda), torch.zeros(2, 4097, device=cuda), 0)
    with pytest.raises(RuntimeError, match="bad argument"):
        manoadapt.adapt_hip(verts, up(w, cuda), 21)
    empty = manoadapt.adapt_hip(verts[:0], up(w, cuda), 9)
    assert tuple(empty[0].shape) == (0, 778, 3) and tuple(empty[1].shape) == (0, 21, 3)
