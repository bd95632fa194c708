"""A residual block's tail with its downsample branch in one kernel each way: ``frozen_bn.bn_add_bn_act`` =
relu(bn(x) + bn_d(xd)) (``mr_bn_add_bn_act_forward`` / ``_backward``, csrc/frozen_bn.hip) against a plain fp64 reference
and against the two ``bn_act`` calls it replaces.

Exact cases: small dyadic operands as in tests/test_gpu_trunk_exact.py (x, xd integers in [-4, 4], gradients integers
in [-3, 3], running means in [-1, 1], biases in [-2, 2], var + eps = 0.25, slopes +-0.5 / +-1 / +-2), so fp64, fp32 and
bf16 hold every intermediate exactly and everything has to agree BIT FOR BIT; the CPU test holds the generator to
z == 0 (the strict ReLU mask) at >= 2 % of the elements."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

EPS = 2.0 ** -10
VAR = 0.25 - EPS          # var + eps = 0.25 exactly, invstd = 2
SLOPES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
FP32, BF16 = torch.float32, torch.bfloat16
_DT = {FP32: "fp32", BF16: "bf16"}

SHAPES = [
    (2, 4, 3, 5),        # 1 channel group
    (2, 128, 3, 3),      # 32 channel groups
    (3, 1024, 10, 10),   # 256 channel groups; 300 workgroups = partial slots > 256: second trip of the finish kernel
    (3, 1024, 27, 27),   # 256; 2187 pixels > 2048 workgroups x 1 row: second grid-stride trip
]
ARRIVALS = ("both", "first", "second")
SMALL = [(2, 4, 3, 5), (2, 128, 3, 3)]

Case = collections.namedtuple("Case", "shape x xd gy gy2 weight bias mean weight_d bias_d mean_d")
Ref = collections.namedtuple("Ref", "y gx gxd gw gb gwd gbd z")
_GRADS = (("gx", "x"), ("gxd", "d"), ("gw", "w"), ("gb", "b"), ("gwd", "W"), ("gbd", "B"))  # field, requires-grad flag


@functools.lru_cache(maxsize=4)
def _case(shape):
    g = torch.Generator().manual_seed(sum(d * 29 ** i for i, d in enumerate(shape)) + 3)
    ints = lambda s, lo, hi: torch.randint(lo, hi + 1, s, generator=g).float()
    C = shape[1]
    slope = lambda: torch.tensor(SLOPES)[torch.randint(0, len(SLOPES), (C,), generator=g)] / 2
    return Case(shape, ints(shape, -4, 4), ints(shape, -4, 4), ints(shape, -3, 3), ints(shape, -3, 3),
                slope(), ints((C,), -2, 2), ints((C,), -1, 1), slope(), ints((C,), -2, 2), ints((C,), -1, 1))


def _grad_out(c, arrival):
    return {"both": c.gy + c.gy2, "first": c.gy, "second": c.gy2}[arrival]


def _reference(c, arrival, dtype=torch.float64):
    """relu(((x - m) * a + b) + ((xd - md) * ad + bd)) from explicit torch ops on the CPU, backward through autograd"""
    t = lambda v: v.to(dtype, copy=True).requires_grad_(True)
    x, xd, w, b, wd, bd = t(c.x), t(c.xd), t(c.weight), t(c.bias), t(c.weight_d), t(c.bias_d)
    invstd = 1.0 / torch.sqrt(torch.full((c.shape[1],), VAR, dtype=dtype) + EPS)
    bc = lambda v: v[None, :, None, None]
    z = ((x - bc(c.mean.to(dtype))) * bc(w * invstd) + bc(b)) + ((xd - bc(c.mean_d.to(dtype))) * bc(wd * invstd) + bc(bd))
    y = F.relu(z)
    y.backward(_grad_out(c, arrival).to(dtype))
    return Ref(y.detach(), x.grad, xd.grad, w.grad, b.grad, wd.grad, bd.grad, z.detach())


@functools.lru_cache(maxsize=4)
def _ref64(shape, arrival):
    return _reference(_case(shape), arrival)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, max |diff| {float(d.max()):g}")


def test_generator_is_exact_and_decides_the_mask_boundary():
    """No GPU: the reference gives the same numbers in fp32 and fp64, y and the activation gradients are bf16 values,
    the channel sums stay below 2^24, and z == 0 at >= 2 % of the elements of every case."""
    for shape in SHAPES:
        c = _case(shape)
        r64, r32 = _reference(c, "both"), _reference(c, "both", FP32)
        for field, a, b in zip(Ref._fields, r32, r64):
            _same(a.double(), b, f"{shape}: fp32 reference {field}")
        for field in ("y", "gx", "gxd"):
            t = getattr(r64, field)
            _same(t.bfloat16().double(), t, f"{shape}: {field} as bf16")
        for field in ("gw", "gb", "gwd", "gbd"):
            assert float(getattr(r64, field).abs().max()) < 2 ** 24
        zero = float((r64.z == 0).double().mean())
        assert zero >= 0.02, f"{shape}: z == 0 at {zero:.3f} of the elements"


# ---- GPU side ----------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """every _lib.call of the test as (name, args)"""
    from handobjectconsist_amd import _lib

    log = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (log.append((name, a)), real_call(name, *a))[1])
    return log


def _module(dev, C, weight, bias, mean, req_w, req_b, var=None, eps=EPS):
    bn = torch.nn.BatchNorm2d(C, eps=eps).to(dev).eval()
    with torch.no_grad():
        bn.weight.copy_(weight)
        bn.bias.copy_(bias)
        bn.running_mean.copy_(mean)
        bn.running_var.fill_(VAR) if var is None else bn.running_var.copy_(var)
    bn.weight.requires_grad_(req_w)
    bn.bias.requires_grad_(req_b)
    return bn


def _put(t, dev, dtype):
    return t.detach().to(dev, dtype, copy=True).contiguous(memory_format=torch.channels_last)


def _run(dev, c, dtype, arrival="both", req="xdwbWB", fused=True, var=None, var_d=None, eps=EPS):
    """forward + backward in the two-output form, fused or as the two bn_act calls the fused op replaces"""
    from handobjectconsist_amd.nn import frozen_bn

    C = c.shape[1]
    bn = _module(dev, C, c.weight, c.bias, c.mean, "w" in req, "b" in req, var, eps)
    bn_d = _module(dev, C, c.weight_d, c.bias_d, c.mean_d, "W" in req, "B" in req, var_d, eps)
    x, xd = _put(c.x, dev, dtype).requires_grad_("x" in req), _put(c.xd, dev, dtype).requires_grad_("d" in req)
    if fused:
        y1, y2 = frozen_bn.bn_add_bn_act(x, bn, xd, bn_d, dup=True)
    else:
        y1, y2 = frozen_bn.bn_act(x, bn, residual=frozen_bn.bn_act(xd, bn_d, relu=False), dup=True)
    assert y1.data_ptr() == y2.data_ptr() and y1.dtype == dtype and y1.is_contiguous(memory_format=torch.channels_last)
    gy, gy2 = _put(c.gy, dev, dtype), _put(c.gy2, dev, dtype)
    if arrival == "both":
        torch.autograd.backward([y1, y2], [gy, gy2])
    elif arrival == "first":
        y1.backward(gy)
    else:
        y2.backward(gy2)
    return Ref(y1.detach(), x.grad, xd.grad, bn.weight.grad, bn.bias.grad, bn_d.weight.grad, bn_d.bias.grad, None)


def _check(got, ref, dev, dtype, req, what):
    _same(got.y, ref.y.to(dev).to(dtype), f"{what}: y")
    for field, flag in _GRADS:
        g, want = getattr(got, field), getattr(ref, field)
        if flag not in req:
            assert g is None, f"{what}: {field} without requires_grad"
        else:
            _same(g, want.to(dev).to(dtype if field in ("gx", "gxd") else FP32), f"{what}: {field}")


def _fused_calls(calls):
    names = [n for n, _ in calls]
    assert names.count("mr_bn_add_bn_act_forward") == 1 and names.count("mr_bn_add_bn_act_backward") == 1, names
    assert not any(n.startswith("mr_bn_act") for n in names), names
    return [a for n, a in calls if n == "mr_bn_add_bn_act_backward"][0]


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return _DT.get(v, str(v))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("arrival", ARRIVALS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_block_tail_exact(cuda, calls, shape, arrival, dtype):
    """y, both input gradients and all four parameter gradients against the fp64 reference, bit for bit, with two
    gradients, one, and each of them None; in fp32 also against the two bn_act calls the op replaces."""
    c = _case(shape)
    got = _run(cuda, c, dtype, arrival)
    second = _fused_calls(calls)[1]  # the grad_y2 argument
    assert (second is not None and second.value) if arrival == "both" else second is None, (arrival, second)
    what = f"bn_add_bn_act {shape} {arrival} {_DT[dtype]}"
    _check(got, _ref64(shape, arrival), cuda, dtype, "xdwbWB", what)
    if dtype == FP32:
        composed = _run(cuda, c, dtype, arrival, fused=False)
        for field in Ref._fields[:-1]:
            _same(getattr(got, field), getattr(composed, field), f"{what} against the composed path: {field}")


# x only (partial NULL, no finish launch), parameters only, bn_d frozen (its two gradients NULL in the finish kernel)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("req", ["x", "wbWB", "xdwb"])
@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_block_tail_with_reduced_requires_grad(cuda, calls, shape, req, dtype):
    c = _case(shape)
    got = _run(cuda, c, dtype, req=req)
    _fused_calls(calls)
    _check(got, _ref64(shape, "both"), cuda, dtype, req, f"bn_add_bn_act {shape} req={req}")


def _randn_case(shape):
    g = torch.Generator().manual_seed(sum(shape) + 2)
    C = shape[1]
    rn = lambda s: torch.randn(s, generator=g)
    bf = lambda t: t.bfloat16().float()   # bf16 values: an fp32 run is the bf16 run's "widened inputs"
    c = Case(shape, bf(rn(shape)), bf(rn(shape)), bf(rn(shape)), bf(rn(shape)), rn(C) * 0.5 + 1.0, rn(C) * 0.3, rn(C) * 0.4,
             rn(C) * 0.5 + 1.0, rn(C) * 0.3, rn(C) * 0.4)
    return c, torch.rand(C, generator=g) * 2 + 0.05, torch.rand(C, generator=g) * 2 + 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 16, 17, 30), (3, 512, 8, 8)], ids=_id)
def test_block_tail_equals_the_composed_path_on_random_data(cuda, shape):
    """fp32, random normal data: same expression shape, same pixel walk and same summation order as the two bn_act
    launches, so every output -- the parameter gradients too -- has the same bits."""
    c, var, var_d = _randn_case(shape)
    got = _run(cuda, c, FP32, var=var, var_d=var_d, eps=1e-5)
    composed = _run(cuda, c, FP32, fused=False, var=var, var_d=var_d, eps=1e-5)
    for field in Ref._fields[:-1]:
        _same(getattr(got, field), getattr(composed, field), f"{shape}: {field}")
    assert float(got.gx.abs().sum()) > 0 and float(got.gwd.abs().sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 16, 17, 30), (3, 512, 8, 8)], ids=_id)
def test_block_tail_bf16_is_the_fp32_kernel_rounded_once(cuda, shape):
    """bf16 activations are widened on load, everything is fp32 arithmetic and only the stores round: y and the input
    gradients equal the fp32 kernel's on the widened inputs, rounded once to bf16 (the normalised downsample branch is
    not rounded in between, unlike the two bn_act calls); the parameter gradients are fp32 sums of the same fp32 terms
    in the same order, so they have the fp32 run's bits."""
    c, var, var_d = _randn_case(shape)
    got = _run(cuda, c, BF16, var=var, var_d=var_d, eps=1e-5)
    ref = _run(cuda, c, FP32, var=var, var_d=var_d, eps=1e-5)
    for field in ("y", "gx", "gxd"):
        _same(getattr(got, field), getattr(ref, field).to(BF16), f"{shape}: {field}")
    for field in ("gw", "gb", "gwd", "gbd"):
        _same(getattr(got, field), getattr(ref, field), f"{shape}: {field}")


def _close(a, b, rel, what):
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.gpu
def test_basic_block_with_downsample_fused_equals_stock_modules(cuda, calls):
    """A BasicBlock with a downsample branch on the fused kernels against the stock modules (the tolerances of
    test_resnet_trunk_fused_equals_stock in tests/test_gpu_nn.py: 1e-4 forward, 2e-3 gradients, relative to the
    scale), and no bn_act launch with relu = 0 -- the downsample branch's own pass -- is left in it."""
    from handobjectconsist_amd.models import synthnet

    torch.manual_seed(0)
    down = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, 2, bias=False), torch.nn.BatchNorm2d(128))
    block = synthnet.BasicBlock(64, 128, 2, down).to(cuda).eval().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    x0 = torch.randn(4, 64, 18, 14, device=cuda).contiguous(memory_format=torch.channels_last)
    w = torch.randn(4, 128, 9, 7, device=cuda)
    out = {}
    for fused in (True, False):
        block.zero_grad(set_to_none=True)
        x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
        del calls[:]
        y = block.forward_fused(x, x) if fused else block.relu(block.bn2(block.conv2(block.relu(block.bn1(block.conv1(x))))) + down(x))
        (y * w).sum().backward()
        out[fused] = (y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in block.named_parameters()})
        if fused:
            names = [n for n, _ in calls]
            assert names.count("mr_bn_add_bn_act_forward") == 1 and names.count("mr_bn_add_bn_act_backward") == 1, names
            # relu is argument 7 of mr_bn_act_forward and 9 of mr_bn_act_backward
            assert not any((n == "mr_bn_act_forward" and a[7] == 0) or (n == "mr_bn_act_backward" and a[9] == 0)
                           for n, a in calls), names
    _close(out[True][0], out[False][0], 1e-4, "block output")
    _close(out[True][1], out[False][1], 2e-3, "grad x")
    for n, gref in out[False][2].items():
        _close(out[True][2][n], gref, 2e-3, f"grad {n}")
