"""The stem with pooled records (``mr_stem_pool_forward`` / ``_backward`` with layout code 2, csrc/stem_pool.hip): the
forward leaves x - mean of every window's arg-max pixel next to its arg-max code, and the backward works from those
records alone -- x is not read, may be NULL and is not kept by the Python layer.

Exact cases: the operands are small dyadic values as in tests/test_gpu_trunk_exact.py (x integers in [-4, 4], gradients
integers in [-3, 3], running_mean in [-1, 1], bias in [-2, 2], var + eps = 0.25, slopes +-0.5 / +-1 / +-2), so fp64,
fp32 and bf16 hold every intermediate exactly, the summation order of the channel sums does not matter and the kernels
have to agree with a plain fp64 reference BIT FOR BIT, no pixel exempt.  The CPU test holds the generator to
z == 0 at >= 2 % of the elements and a repeated positive maximum in >= 10 % of the windows.

Random normal data: layout 2 against layout 1 -- y, grad_x and the arg-max codes bit for bit; grad_weight / grad_bias
(whose fp32 summation order differs between the layouts) against an fp64 sum of the same fp32 terms within the worst
case of any fp32 summation order, n * 2^-24 * sum |term| per channel for n terms."""
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
POISON = 0xA5
TAIL = 64                 # poison bytes behind every output buffer

# (shape, arrival): what each shape reaches is said next to it.  A thread of the backward owns a 2 x 2 quad of input
# pixels (rows 2 q - 1, 2 q), a thread of the forward a 2 x 2 quad of pooled pixels; 256 / (C / 4) quads per workgroup.
EXACT = [
    ((2, 4, 35, 70), "both"),      # odd H, quads and windows cut by the bottom and right edges, batch boundary
    ((2, 64, 17, 31), "both"),     # 16 channel groups, the trunk's form
    ((1, 1024, 65, 65), "both"),   # one quad per workgroup
    ((1, 256, 129, 129), "both"),  # 4 quads per workgroup, 1057 workgroups
    ((2, 4, 2, 3), "both"),        # smallest non-trivial image
    ((2, 8, 1, 1), "both"),        # one-pixel image
    ((2, 4, 35, 70), "first"),     # single-gradient form
    ((2, 4, 35, 70), "second"),
]
# more quads than 4096 workgroups x 1: second grid-stride trip of the forward (65 x 65 pooled quads) and of the backward
# (129 x 129 input quads).  67 M elements, so it is compared with layout 1 on the GPU, not with the CPU reference.
TWO_TRIPS = (1, 1024, 257, 257)
RANDN = [(5, 16, 17, 30), (6, 64, 32, 32)]

# seeds of the two tiny shapes, chosen so that even they meet the generator conditions of the CPU test
_SEEDS = {(2, 4, 2, 3): 6, (2, 8, 1, 1): 6}

Case = collections.namedtuple("Case", "shape x gy gy2 weight bias mean")
Ref = collections.namedtuple("Ref", "y gx gw gb z")
Out = collections.namedtuple("Out", "y gx gw gb d code")


def _pooled(shape):
    N, C, H, W = shape
    return (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


def _draw(shape, g, device="cpu"):
    ints = lambda s, lo, hi: torch.randint(lo, hi + 1, s, generator=g, device=device).float()
    C = shape[1]
    slopes = torch.tensor(SLOPES, device=device)[torch.randint(0, len(SLOPES), (C,), generator=g, device=device)]
    return Case(shape, ints(shape, -4, 4), ints(_pooled(shape), -3, 3), ints(_pooled(shape), -3, 3), slopes / 2,
                ints((C,), -2, 2), ints((C,), -1, 1))


@functools.lru_cache(maxsize=4)
def _case(shape):
    seed = _SEEDS.get(shape, sum(d * 37 ** i for i, d in enumerate(shape)) + 5)
    return _draw(shape, torch.Generator().manual_seed(seed))


def _grad_out(c, arrival):
    return {"both": c.gy + c.gy2, "first": c.gy, "second": c.gy2}[arrival]


def _reference(c, arrival, dtype=torch.float64):
    """(x - mean) * (weight / sqrt(var + eps)) + bias -> relu -> max_pool2d(3, 2, 1) from explicit torch ops on the CPU,
    backward through autograd with the sum of the gradients that arrive"""
    x = c.x.to(dtype, copy=True).requires_grad_(True)
    w, b = c.weight.to(dtype, copy=True).requires_grad_(True), c.bias.to(dtype, copy=True).requires_grad_(True)
    a = w / torch.sqrt(torch.full_like(w, VAR).detach() + EPS)
    z = (x - c.mean.to(dtype)[None, :, None, None]) * a[None, :, None, None] + b[None, :, None, None]
    y = F.max_pool2d(F.relu(z), 3, 2, 1)
    y.backward(_grad_out(c, arrival).to(dtype))
    return Ref(y.detach(), x.grad, w.grad, b.grad, z.detach())


@functools.lru_cache(maxsize=4)
def _ref64(shape, arrival):
    return _reference(_case(shape), arrival)


def _tie_share(z):
    """share of the 3 x 3 / stride 2 / padding 1 windows of relu(z) whose maximum is positive and held more than once"""
    N, C, H, W = z.shape
    v = F.pad(F.relu(z), (1, 1, 1, 1), value=float("-inf")).reshape(N * C, 1, H + 2, W + 2)
    win = F.unfold(v, 3, stride=2)
    mx = win.max(1, keepdim=True).values
    return float((((win == mx).sum(1, keepdim=True) > 1) & (mx > 0)).double().mean())


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, max |diff| {float(d.max()):g}")


def test_generator_is_exact_and_decides_ties_and_the_mask_boundary():
    """No GPU: on every exact case the reference gives the same numbers in fp32 and fp64, outputs and activation
    gradients are bf16 values, the channel sums stay below 2^24, z == 0 at >= 2 % of the elements and >= 10 % of the
    windows hold a repeated positive maximum (all but the one-pixel image, whose window holds a single value)."""
    for shape in dict.fromkeys(s for s, _ in EXACT):
        c = _case(shape)
        for arrival in sorted({a for s, a in EXACT if s == shape}):
            r64, r32 = _reference(c, arrival), _reference(c, arrival, FP32)
            for field, a, b in zip(Ref._fields, r32, r64):
                _same(a.double(), b, f"{shape} {arrival}: fp32 reference {field}")
            for field in ("y", "gx"):
                t = getattr(r64, field)
                _same(t.bfloat16().double(), t, f"{shape} {arrival}: {field} as bf16")
            assert float(r64.gw.abs().max()) < 2 ** 24 and float(r64.gb.abs().max()) < 2 ** 24
        zero = float((r64.z == 0).double().mean())
        assert zero >= 0.02, f"{shape}: z == 0 at {zero:.3f} of the elements"
        if shape[2] * shape[3] > 1:
            ties = _tie_share(r64.z)
            assert ties >= 0.10, f"{shape}: {ties:.3f} of the windows hold a repeated positive maximum"


# ---- GPU side ----------------------------------------------------------------------------------------------------
def _poisoned(nbytes, dev):
    """a byte buffer of ``nbytes`` + TAIL poison bytes; the caller's data goes into the first ``nbytes``"""
    return torch.full((nbytes + TAIL,), POISON, dtype=torch.uint8, device=dev)


def _tail_intact(buf, what):
    assert bool((buf[-TAIL:] == POISON).all()), f"{what}: bytes behind the buffer were written"


def _nhwc(t, dev, dtype):
    return t.to(dev).permute(0, 2, 3, 1).contiguous().to(dtype)


def _raw(dev, c, dtype, layout, grads, params=True, var=None, eps=EPS):
    """One forward + backward through the C entry points on NHWC buffers in layout 1 or 2.  ``grads``: the one or two
    pooled gradients (NCHW tensors).  Layout 2: x is overwritten with NaN after the forward and the backward gets
    x = NULL.  Every output buffer has poison bytes behind it, checked at the end.  Results as NCHW tensors."""
    from handobjectconsist_amd import _lib

    P, st = _lib.ptr, _lib.stream_ptr(dev)
    N, C, H, W = c.shape
    _, _, OH, OW = _pooled(c.shape)
    esz = 4 if dtype == FP32 else 2
    code = 0 if dtype == FP32 else 1
    x = _nhwc(c.x, dev, dtype)
    w, b, m = (t.to(dev).float().contiguous() for t in (c.weight, c.bias, c.mean))
    v = torch.full((C,), VAR, device=dev) if var is None else var.to(dev).float().contiguous()
    pooled = N * OH * OW * C
    ybuf, gxbuf = _poisoned(pooled * esz, dev), _poisoned(N * H * W * C * esz, dev)
    rbytes = int(_lib.load().mr_stem_pool_records_bytes(N, C, H, W)) if layout == 2 else pooled
    if layout == 2:
        assert rbytes == pooled * 4 + (pooled + 15) // 16 * 16
    rbuf = _poisoned(rbytes, dev)
    assert _lib.call("mr_stem_pool_forward", P(x), P(w), P(b), P(m), P(v), eps, code, layout, P(ybuf), P(rbuf), N, C, H, W, st) == 0
    gs = [_nhwc(g, dev, dtype) for g in grads]
    g2 = gs[1] if len(gs) == 2 else None
    if layout == 2:
        x.fill_(float("nan"))
        x = None
    gw, gb = (torch.empty(C, device=dev), torch.empty(C, device=dev)) if params else (None, None)
    wbytes = int(_lib.load().mr_stem_pool_backward_workspace_bytes(N, C, H, W))
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev) if params else None
    assert _lib.call("mr_stem_pool_backward", P(gs[0]), P(g2), P(x), P(rbuf), P(w), P(b), P(m), P(v), eps, code, layout,
                     P(gxbuf), P(gw), P(gb), P(work), wbytes, N, C, H, W, st) == 0
    torch.cuda.synchronize(dev)
    for buf, what in ((ybuf, "y"), (gxbuf, "grad_x"), (rbuf, "records")):
        _tail_intact(buf, f"layout {layout} {c.shape}: {what}")
    y = ybuf[:pooled * esz].view(dtype).view(N, OH, OW, C).permute(0, 3, 1, 2)
    gx = gxbuf[:N * H * W * C * esz].view(dtype).view(N, H, W, C).permute(0, 3, 1, 2)
    if layout == 2:
        d = rbuf[:pooled * 4].view(FP32).view(N, OH, OW, C).permute(0, 3, 1, 2)
        am = rbuf[pooled * 4:pooled * 5].view(N, OH, OW, C).permute(0, 3, 1, 2)
    else:
        d, am = None, rbuf[:pooled].view(N, OH, OW, C).permute(0, 3, 1, 2)
    return Out(y, gx, gw, gb, d, am)


def _check_records(out, c, dev, dtype, what):
    """the d plane is x - mean of the pixel the code names (kh * 3 + kw, window origin 2 o - 1), exactly, and that pixel
    lies inside the image"""
    N, C, H, W = c.shape
    _, _, OH, OW = _pooled(c.shape)
    code = out.code.long()
    assert int(code.max()) <= 8, what
    oy = torch.arange(OH, device=dev)[None, None, :, None]
    ox = torch.arange(OW, device=dev)[None, None, None, :]
    iy, ix = 2 * oy - 1 + code // 3, 2 * ox - 1 + code % 3
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), f"{what}: a code names a pixel outside the image"
    x = c.x.to(dev).to(dtype).float()                       # the values the kernel widened
    picked = x.reshape(N, C, H * W).gather(2, (iy * W + ix).reshape(N, C, OH * OW)).reshape(N, C, OH, OW)
    _same(out.d.contiguous(), (picked - c.mean.to(dev).float()[None, :, None, None]).contiguous(), f"{what}: record d")


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return _DT.get(v, str(v))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("shape,arrival", EXACT, ids=_id)
def test_records_exact(cuda, shape, arrival, dtype):
    """Layout 2 through the entry points, x = NULL in the backward: y, grad_x, grad_weight and grad_bias against the
    fp64 reference bit for bit; the records hold x - mean of the coded pixel; nothing is written behind a buffer."""
    c, ref = _case(shape), _ref64(shape, arrival)
    grads = {"both": (c.gy, c.gy2), "first": (c.gy,), "second": (c.gy2,)}[arrival]
    out = _raw(cuda, c, dtype, 2, grads)
    what = f"records {shape} {arrival} {_DT[dtype]}"
    _same(out.y.contiguous(), ref.y.to(cuda).to(dtype), f"{what}: y")
    _same(out.gx.contiguous(), ref.gx.to(cuda).to(dtype), f"{what}: grad_x")
    _same(out.gw, ref.gw.to(cuda).float(), f"{what}: grad_weight")
    _same(out.gb, ref.gb.to(cuda).float(), f"{what}: grad_bias")
    _check_records(out, c, cuda, dtype, what)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
def test_records_exact_without_parameter_gradients(cuda, dtype):
    """grad_weight = grad_bias = workspace = NULL: no partial sums, same grad_x"""
    shape = (2, 4, 35, 70)
    c, ref = _case(shape), _ref64(shape, "both")
    out = _raw(cuda, c, dtype, 2, (c.gy, c.gy2), params=False)
    _same(out.gx.contiguous(), ref.gx.to(cuda).to(dtype), "grad_x without parameter gradients")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
def test_second_grid_stride_trip_equals_layout_1(cuda, dtype):
    """TWO_TRIPS: both kernels of layout 2 walk their quads in more than one trip.  Exact data drawn on the GPU, so
    everything -- the channel sums too -- has to equal layout 1 bit for bit (layout 1 itself is held to the fp64
    reference by tests/test_gpu_trunk_exact.py)."""
    g = torch.Generator(device=cuda).manual_seed(11)
    c = _draw(TWO_TRIPS, g, cuda)
    a = c.weight * 2
    z = (c.x[:, :16] - c.mean[None, :16, None, None]) * a[None, :16, None, None] + c.bias[None, :16, None, None]
    assert float((z == 0).float().mean()) >= 0.02 and _tie_share(z[:, :, :65, :65].cpu()) >= 0.10
    one, two = _raw(cuda, c, dtype, 1, (c.gy, c.gy2)), _raw(cuda, c, dtype, 2, (c.gy, c.gy2))
    for field in ("y", "gx", "gw", "gb", "code"):
        _same(getattr(two, field), getattr(one, field), f"{TWO_TRIPS} {_DT[dtype]}: {field}")
    assert float(one.gx.float().abs().sum()) > 0 and float(one.gw.abs().sum()) > 0


def _randn_case(shape):
    g = torch.Generator().manual_seed(sum(shape) + 1)
    C = shape[1]
    rn = lambda s: torch.randn(s, generator=g)
    bf = lambda t: t.bfloat16().float()     # bf16 values: the same data for both activation types
    c = Case(shape, bf(rn(shape)), bf(rn(_pooled(shape))), bf(rn(_pooled(shape))), rn(C) * 0.5 + 1.0, rn(C) * 0.3, rn(C) * 0.4)
    return c, torch.rand(C, generator=g) * 2 + 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("shape", RANDN, ids=_id)
def test_layout_2_against_layout_1_on_random_data(cuda, shape, dtype):
    """y, grad_x and the arg-max codes equal layout 1's bit for bit.  grad_bias = sum s and grad_weight = invstd * sum
    fp32(s * d) over the windows, s = active ? fp32(gy + gy2) : 0: against the fp64 sum of those same fp32 terms, within
    n * 2^-24 * sum |term| per channel (n = N * OH * OW terms) -- the worst case of any fp32 summation order; a dropped
    or doubled term is what the exact cases catch."""
    c, var = _randn_case(shape)
    eps = 1e-5
    one = _raw(cuda, c, dtype, 1, (c.gy, c.gy2), var=var, eps=eps)
    two = _raw(cuda, c, dtype, 2, (c.gy, c.gy2), var=var, eps=eps)
    for field in ("y", "gx", "code"):
        _same(getattr(two, field), getattr(one, field), f"{shape} {_DT[dtype]}: {field}")
    _check_records(two, c, cuda, dtype, f"{shape} {_DT[dtype]}")
    N, C, OH, OW = _pooled(shape)
    n = N * OH * OW
    g = (c.gy + c.gy2).to(cuda)                              # fp32 add of bf16 values, as the kernel's
    s = torch.where(two.y.float() > 0, g, torch.zeros_like(g))   # y > 0 <=> z > 0 at the arg-max pixel
    sd = s * two.d                                           # fp32 products, as the kernel's
    invstd = 1.0 / torch.sqrt((var.float() + torch.tensor(eps, dtype=FP32)).double()).to(cuda)
    want_b, want_w = s.double().sum((0, 2, 3)), sd.double().sum((0, 2, 3)) * invstd
    bound_b = n * 2.0 ** -24 * s.double().abs().sum((0, 2, 3))
    bound_w = n * 2.0 ** -24 * sd.double().abs().sum((0, 2, 3)) * invstd
    err_b, err_w = (two.gb.double() - want_b).abs(), (two.gw.double() - want_w).abs()
    share = lambda err, bound: float((err / bound.clamp_min(1e-300)).max())   # (a channel whose windows are all inactive: 0 / 0)
    print(f"grad_bias err / bound max {share(err_b, bound_b):.3e}, grad_weight {share(err_w, bound_w):.3e}")
    assert bool((err_b <= bound_b).all()), f"grad_bias: max err / bound {share(err_b, bound_b):.3e}"
    assert bool((err_w <= bound_w).all()), f"grad_weight: max err / bound {share(err_w, bound_w):.3e}"


# ---- the Python layer ----------------------------------------------------------------------------------------------
def _module(dev, c):
    bn = torch.nn.BatchNorm2d(c.shape[1], eps=EPS).to(dev).eval()
    with torch.no_grad():
        bn.weight.copy_(c.weight)
        bn.bias.copy_(c.bias)
        bn.running_mean.copy_(c.mean)
        bn.running_var.fill_(VAR)
    return bn


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
def test_python_layer_runs_layout_2_and_does_not_keep_x(cuda, monkeypatch, dtype):
    """frozen_bn.stem_pool on a channels-last activation: layout code 2 both ways, x = NULL in the backward, and the
    convolution output is neither kept nor read after the forward -- it is overwritten with NaN and freed before the
    backward, the allocator gets its bytes back, and the result still equals the fp64 reference bit for bit."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.nn import frozen_bn

    shape = (2, 64, 17, 31)
    c, ref = _case(shape), _ref64(shape, "both")
    log = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (log.append((name, a)), real_call(name, *a))[1])
    bn = _module(cuda, c)
    leaf = c.x.to(cuda, dtype).requires_grad_(True)                       # NCHW leaf
    x = leaf.contiguous(memory_format=torch.channels_last)                # the activation the stem gets: a new buffer
    assert x.data_ptr() != leaf.data_ptr()
    y1, y2 = frozen_bn.stem_pool(x, bn, dup=True)
    nbytes = x.numel() * x.element_size()
    x.detach().fill_(float("nan"))
    torch.cuda.synchronize(cuda)
    before = torch.cuda.memory_allocated(cuda)
    del x
    assert torch.cuda.memory_allocated(cuda) <= before - nbytes, "the stem's autograd node keeps the convolution output"
    fmt = torch.channels_last
    torch.autograd.backward([y1, y2], [c.gy.to(cuda, dtype).contiguous(memory_format=fmt), c.gy2.to(cuda, dtype).contiguous(memory_format=fmt)])
    fwd = [a for n, a in log if n == "mr_stem_pool_forward"]
    bwd = [a for n, a in log if n == "mr_stem_pool_backward"]
    assert len(fwd) == 1 and len(bwd) == 1, [n for n, _ in log]
    assert fwd[0][7] == 2 and bwd[0][10] == 2, "layout code"
    assert bwd[0][2] is None, "x of the backward"
    _same(y1.detach(), ref.y.to(cuda).to(dtype), "y")
    _same(leaf.grad, ref.gx.to(cuda).to(dtype), "grad_x")
    _same(bn.weight.grad, ref.gw.to(cuda).float(), "grad_weight")
    _same(bn.bias.grad, ref.gb.to(cuda).float(), "grad_bias")
