"""The trunk glue kernels (csrc/frozen_bn.hip, csrc/stem_pool.hip) in the form the trainer launches -- two output
gradients summed on load (``dup=True``) -- on inputs where the operation is EXACT.

Every operand is a small dyadic value: x, residual integers in [-4, 4], the gradients integers in [-3, 3],
running_mean in [-1, 1], bias in [-2, 2], var + eps = 0.25 (invstd = 2) and weight = a / 2 with the slope a in
{+-0.5, +-1, +-2}.  Then (x - mean) * a + b (+ residual), the ReLU, the pooling, g * a and both channel sums are
multiples of 0.25 far below 2^24 (and, for the activations, within bf16's 8 significant bits): fp64, fp32 and bf16
hold every intermediate exactly, summation order does not matter, and the plain fp64 reference below, the stock
modules and every kernel variant have to agree BIT FOR BIT -- no exempt pixel, no tolerance.  z == 0 (the strict
ReLU mask) and repeated positive maxima in a pooling window (stock rule: first strictly greater value in (kh, kw)
order) occur all over such data; the CPU test holds the generator to that.

The rounding of the two-gradient form (which exact data cannot show) and misaligned channels-last operands are
tested on random normal data at the end."""
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

# ---- shapes: the smallest that reach each launch-geometry branch -------------------------------------------------
BN_NCHW = [
    (3, 8, 4, 4),        # vector path
    (3, 5, 3, 5),        # scalar path (HW % 4 != 0)
    (6, 1024, 2, 2),     # split = 4 < N: sample ranges 1 / 2 / 1 / 2
    (300, 4, 1, 4),      # split = 300 > 256: second trip of bn_finish_kernel<2>
]
BN_CL_FALLBACK = (5, 2048, 1, 4)   # channels-last input with C > 1024: NCHW kernels through _layout
BN_CL = [
    (2, 4, 3, 5),        # 1 group of 4 channels
    (2, 8, 3, 5),        # 2
    (2, 64, 5, 7),       # 16
    (2, 256, 3, 3),      # 64
    (2, 512, 3, 3),      # 128
    (3, 1024, 10, 10),   # 256; 300 workgroups = partial slots > 256
    (3, 1024, 27, 27),   # 256; 2187 pixels > 2048 workgroups x 1 row: second grid-stride trip
]
STEM_NCHW = [
    (2, 3, 35, 70),      # two tiles each way, W % 4 != 0, odd H
    (2, 4, 36, 72),      # vector path across tile seams
    (70, 2, 33, 65),     # N * tiles = 280 > 256 slots: second trip of bn_finish_kernel<2> (the stem's slots)
    (2, 3, 1, 1),
    (1, 2, 2, 3),
]
STEM_CL = [
    (2, 4, 35, 70),
    (2, 64, 17, 31),
    (1, 1024, 65, 65),   # 4225 input pixels > 4096 workgroups x 1 row
    (1, 256, 129, 129),  # rows = 4: 16641 input pixels > 16384 (two trips), the forward's 4225 pooled pixels are not
    (2, 4, 1, 1),        # channels-last == contiguous here: the NCHW kernels
]
RELU_RES = [(True, False), (True, True), (False, False), (False, True)]
SMALL_BN = [((3, 8, 4, 4), False), ((3, 5, 3, 5), False), ((2, 8, 3, 5), True)]
SMALL_STEM = [((2, 3, 35, 70), False), ((2, 4, 35, 70), True)]

Case = collections.namedtuple("Case", "op shape relu x r gy gy2 weight bias mean")
Ref = collections.namedtuple("Ref", "y gx gr gw gb z")

# seeds of the three tiny stem shapes (6 - 8 elements), chosen so that even they meet the generator conditions of the CPU
# test: z == 0 somewhere and, where a window holds more than one pixel, a repeated positive maximum in one
_SEEDS = {("stem", (2, 3, 1, 1), True, False): 8, ("stem", (1, 2, 2, 3), True, False): 6,
          ("stem", (2, 4, 1, 1), True, False): 2}


def _seed(op, shape, relu, with_res):
    key = (op, shape, relu, with_res)
    return _SEEDS.get(key, sum(d * 31 ** i for i, d in enumerate(shape)) + 7 * relu + 13 * with_res + (op == "stem"))


def _pooled(shape):
    N, C, H, W = shape
    return (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


@functools.lru_cache(maxsize=6)
def _case(op, shape, relu=True, with_res=False):
    """The exact operands (CPU, fp32 -- every value is a small dyadic number, exact in any float type)."""
    g = torch.Generator().manual_seed(_seed(op, shape, relu, with_res))
    ints = lambda s, lo, hi: torch.randint(lo, hi + 1, s, generator=g).float()
    C = shape[1]
    oshape = _pooled(shape) if op == "stem" else shape
    slopes = torch.tensor(SLOPES)[torch.randint(0, len(SLOPES), (C,), generator=g)]
    return Case(op, shape, relu, ints(shape, -4, 4), ints(shape, -4, 4) if with_res else None, ints(oshape, -3, 3),
                ints(oshape, -3, 3), slopes / 2, ints((C,), -2, 2), ints((C,), -1, 1))


def _grad_out(c, arrival):
    return {"both": c.gy + c.gy2, "first": c.gy, "second": c.gy2}[arrival]


def _reference(c, arrival="both", dtype=torch.float64):
    """z = (x - mean) * (weight / sqrt(var + eps)) + bias [+ residual] -> relu -> max_pool2d(3, 2, 1) from explicit
    torch ops on the CPU (no F.batch_norm: a library's reciprocal square root is not known to be exact), backward
    through autograd with the sum of the gradients that arrive."""
    x = c.x.to(dtype, copy=True).requires_grad_(True)
    r = c.r.to(dtype, copy=True).requires_grad_(True) if c.r is not None else None
    w, b = c.weight.to(dtype, copy=True).requires_grad_(True), c.bias.to(dtype, copy=True).requires_grad_(True)
    var = torch.full_like(w, VAR).detach()
    a = w / torch.sqrt(var + EPS)
    z = (x - c.mean.to(dtype)[None, :, None, None]) * a[None, :, None, None] + b[None, :, None, None]
    if r is not None:
        z = z + r
    y = F.relu(z) if c.relu else z
    if c.op == "stem":
        y = F.max_pool2d(y, 3, 2, 1)
    y.backward(_grad_out(c, arrival).to(dtype))
    return Ref(y.detach(), x.grad, None if r is None else r.grad, w.grad, b.grad, z.detach())


@functools.lru_cache(maxsize=6)
def _ref64(op, shape, relu, with_res, arrival):
    return _reference(_case(op, shape, relu, with_res), arrival)


def _stock(c, arrival, dtype):
    """The stock modules the kernels replace: BatchNorm2d(eps = 2^-10).eval() + relu + max_pool2d."""
    C = c.shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=EPS).to(dtype).eval()
    with torch.no_grad():
        bn.weight.copy_(c.weight)
        bn.bias.copy_(c.bias)
        bn.running_mean.copy_(c.mean)
        bn.running_var.fill_(VAR)
    x = c.x.to(dtype, copy=True).requires_grad_(True)
    r = c.r.to(dtype, copy=True).requires_grad_(True) if c.r is not None else None
    z = bn(x)
    if r is not None:
        z = z + r
    y = F.relu(z) if c.relu else z
    if c.op == "stem":
        y = F.max_pool2d(y, 3, 2, 1)
    y.backward(_grad_out(c, arrival).to(dtype))
    return Ref(y.detach(), x.grad, None if r is None else r.grad, bn.weight.grad, bn.bias.grad, z.detach())


def _tie_share(z):
    """Share of the 3 x 3 / stride 2 / padding 1 windows of relu(z) whose maximum is positive and held more than once."""
    N, C, H, W = z.shape
    v = F.pad(F.relu(z), (1, 1, 1, 1), value=float("-inf")).reshape(N * C, 1, H + 2, W + 2)
    win = F.unfold(v, 3, stride=2)                      # [N * C, 9, windows]
    mx = win.max(1, keepdim=True).values
    return float((((win == mx).sum(1, keepdim=True) > 1) & (mx > 0)).double().mean())


def _all_cases():
    for shape in BN_NCHW + [BN_CL_FALLBACK] + BN_CL:
        for relu, with_res in RELU_RES:
            yield "bn", shape, relu, with_res
    for shape in STEM_NCHW + STEM_CL:
        yield "stem", shape, True, False


def _same(got, want, what):
    """torch.equal with the figures in the message"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, max |diff| {float(d.max()):g}")


def test_generator_is_exact_in_fp32_fp64_bf16_and_against_the_stock_modules():
    """Keeps the generator honest (no GPU): on every case of this file the reference gives the same numbers in fp32 and
    fp64, so do the stock modules, the outputs and activation gradients are bf16 values, and the data decide the ReLU
    boundary (z == 0 at >= 2 % of the elements) and the pooling tie rule (>= 10 % of the windows hold their positive
    maximum more than once; all but the one-pixel images, where a window holds a single value)."""
    for op, shape, relu, with_res in _all_cases():
        c = _case(op, shape, relu, with_res)
        what = f"{op} {shape} relu={relu} res={with_res}"
        r64 = _reference(c, "both", torch.float64)
        for other, name in ((_reference(c, "both", torch.float32), "fp32 reference"),
                            (_stock(c, "both", torch.float32), "stock fp32 modules")):
            for field, a, b in zip(Ref._fields, other, r64):
                assert (a is None) == (b is None)
                if a is not None:
                    _same(a.double(), b, f"{what}: {name} {field}")
        if c.x.numel() <= 100000:       # the fp64 stock modules too where that is cheap
            for field, a, b in zip(Ref._fields, _stock(c, "both", torch.float64), r64):
                if a is not None:
                    _same(a, b, f"{what}: stock fp64 modules {field}")
        for field in ("y", "gx", "gr"):
            t = getattr(r64, field)
            if t is not None:
                _same(t.bfloat16().double(), t, f"{what}: {field} as bf16")
        assert float(r64.gw.abs().max()) < 2 ** 24 and float(r64.gb.abs().max()) < 2 ** 24
        zero = float((r64.z == 0).double().mean())
        assert zero >= 0.02, f"{what}: z == 0 at {zero:.3f} of the elements"
        if op == "stem" and shape[2] * shape[3] > 1:    # (the window of a one-pixel image holds one value: no tie to decide)
            ties = _tie_share(r64.z)
            assert ties >= 0.10, f"{what}: {ties:.3f} of the windows hold a repeated positive maximum"
        for arrival in ("first", "second"):              # the single-gradient references the GPU tests use
            if any(shape == s for s, _ in (SMALL_BN if op == "bn" else SMALL_STEM)):
                a, b = _reference(c, arrival, torch.float32), _reference(c, arrival, torch.float64)
                _same(a.gx.double(), b.gx, f"{what}: fp32 reference gx, {arrival} gradient only")


# ---- GPU side ----------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """every _lib.call of the test as (name, args)"""
    from handobjectconsist_amd import _lib

    log = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (log.append((name, a)), real_call(name, *a))[1])
    return log


def _module(dev, C, weight, bias, mean, var=None, req="wb"):
    bn = torch.nn.BatchNorm2d(C, eps=EPS).to(dev).eval()
    with torch.no_grad():
        bn.weight.copy_(weight)
        bn.bias.copy_(bias)
        bn.running_mean.copy_(mean)
        bn.running_var.fill_(VAR) if var is None else bn.running_var.copy_(var)
    bn.weight.requires_grad_("w" in req)
    bn.bias.requires_grad_("b" in req)
    return bn


def _put(t, dev, dtype, cl, offset=False):
    """``t`` on the device in the layout under test; ``offset``: as a dense view that starts one element (4 bytes fp32,
    2 bytes bf16) into a larger buffer, so its pointer is off the 16 / 8-byte boundary of a 4-element access"""
    t = t.detach().to(dev, dtype, copy=True).contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    if offset:
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=dev)
        N, C, H, W = t.shape
        v = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2) if cl else buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % (4 * t.element_size()) != 0 and v.stride() == t.stride()
        t = v
    return t


def _backward_calls(calls, op):
    name = "mr_bn_act_backward" if op == "bn" else "mr_stem_pool_backward"
    return [a for n, a in calls if n == name]


def _run(dev, calls, c, dtype, cl, arrival="both", req="xrwb", offset=()):
    """One forward + backward of the fused op in its two-output form; returns what it produced."""
    from handobjectconsist_amd.nn import frozen_bn

    bn = _module(dev, c.shape[1], c.weight, c.bias, c.mean, req=req)
    x = _put(c.x, dev, dtype, cl, "x" in offset).requires_grad_("x" in req)
    r = _put(c.r, dev, dtype, cl, "r" in offset).requires_grad_("r" in req) if c.r is not None else None
    del calls[:]
    if c.op == "bn":
        y1, y2 = frozen_bn.bn_act(x, bn, residual=r, relu=c.relu, dup=True)
    else:
        y1, y2 = frozen_bn.stem_pool(x, bn, dup=True)
    assert y1.data_ptr() == y2.data_ptr() and y1.dtype == dtype
    gy_cl = cl and y1.is_contiguous(memory_format=torch.channels_last)
    gy, gy2 = _put(c.gy, dev, dtype, gy_cl, "gy" in offset), _put(c.gy2, dev, dtype, gy_cl, "gy2" in offset)
    if arrival == "both":
        torch.autograd.backward([y1, y2], [gy, gy2])
    elif arrival == "first":
        y1.backward(gy)
    else:
        y2.backward(gy2)
    bw = _backward_calls(calls, c.op)
    assert len(bw) == 1, [n for n, _ in calls]
    second = bw[0][1]  # the grad_y2 argument
    assert (second is not None and second.value) if arrival == "both" else second is None, (arrival, second)
    if "gy2" in offset and not gy_cl:  # the NCHW kernels get the misaligned pointer itself (their scalar path)
        assert second.value == gy2.data_ptr() and second.value % (4 * gy2.element_size()) != 0
    return Ref(y1.detach(), x.grad, None if r is None else r.grad, bn.weight.grad, bn.bias.grad, None)


def _check(got, ref, dev, dtype, req, what):
    _same(got.y, ref.y.to(dev).to(dtype), f"{what}: y")
    for field, flag, cast in (("gx", "x", dtype), ("gr", "r", dtype), ("gw", "w", FP32), ("gb", "b", FP32)):
        g, want = getattr(got, field), getattr(ref, field)
        if flag not in req or want is None:
            assert g is None, f"{what}: {field} without requires_grad"
        else:
            _same(g, want.to(dev).to(cast), f"{what}: {field}")


_BN_CASES = ([(s, False, False) for s in BN_NCHW] + [((3, 8, 4, 4), False, True), (BN_CL_FALLBACK, True, False)] +
             [(s, True, False) for s in BN_CL])


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return _DT.get(v, str(v))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cl,gy2_offset,relu,with_res,dtype",
                         [(s, cl, off, relu, res, dt) for s, cl, off in _BN_CASES for relu, res in RELU_RES
                          for dt in (FP32, BF16)], ids=_id)
def test_bn_act_two_gradients_exact(cuda, calls, shape, cl, gy2_offset, relu, with_res, dtype):
    """bn_act(dup=True) with both gradients against the fp64 reference, bit for bit, at every launch-geometry branch
    (see the shape lists); ``gy2_offset``: grad_y2 4 bytes off the vector alignment, so the NCHW kernel takes its
    scalar path although HW % 4 == 0."""
    c = _case("bn", shape, relu, with_res)
    got = _run(cuda, calls, c, dtype, cl, offset=("gy2",) if gy2_offset else ())
    if cl:  # the layout the test means to reach: channels-last kernels, or NCHW for what _layout sends there
        assert got.y.is_contiguous(memory_format=torch.channels_last) == (shape != BN_CL_FALLBACK)
    _check(got, _ref64("bn", shape, relu, with_res, "both"), cuda, dtype, "xrwb", f"bn_act {shape} cl={cl}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cl,dtype", [(s, False, dt) for s in STEM_NCHW for dt in (FP32, BF16)] +
                         [(s, True, dt) for s in STEM_CL for dt in (FP32, BF16)], ids=_id)
def test_stem_pool_two_gradients_exact(cuda, calls, shape, cl, dtype):
    """stem_pool(dup=True) with both gradients against the fp64 reference, bit for bit: the data hold repeated positive
    maxima in >= 10 % of the windows and z == 0 in >= 2 % of the pixels, so the tie rule and the strict ReLU mask are
    decided by the data and no pixel is exempt."""
    c = _case("stem", shape)
    got = _run(cuda, calls, c, dtype, cl)
    _check(got, _ref64("stem", shape, True, False, "both"), cuda, dtype, "xwb", f"stem_pool {shape} cl={cl}")


@pytest.mark.gpu
@pytest.mark.parametrize("arrival", ["first", "second"])
@pytest.mark.parametrize("op,shape,cl,relu,with_res,dtype",
                         [("bn", s, cl, relu, res, dt) for s, cl in SMALL_BN for relu, res in ((True, True), (False, False))
                          for dt in (FP32, BF16)] +
                         [("stem", s, cl, True, False, dt) for s, cl in SMALL_STEM for dt in (FP32, BF16)], ids=_id)
def test_one_of_the_two_gradients_arrives(cuda, calls, op, shape, cl, relu, with_res, dtype, arrival):
    """Only one consumer of the duplicated activation sends a gradient: the other arrives as None (``second``: the swap
    in ``backward``) and the kernel runs in its single-gradient form."""
    c = _case(op, shape, relu, with_res)
    got = _run(cuda, calls, c, dtype, cl, arrival=arrival)
    _check(got, _ref64(op, shape, relu, with_res, arrival), cuda, dtype, "xrwb", f"{op} {shape} cl={cl} {arrival}")


# what requires a gradient: x alone (partial, grad_residual NULL), the weight alone (grad_bias NULL in the finish
# kernel), the bias alone, neither parameter (partial NULL), a residual that takes no gradient (grad_residual NULL)
@pytest.mark.gpu
@pytest.mark.parametrize("req", ["x", "w", "b", "xr", "xwb"])
@pytest.mark.parametrize("op,shape,cl,dtype", [("bn", s, cl, dt) for s, cl in SMALL_BN for dt in (FP32, BF16)] +
                         [("stem", s, cl, dt) for s, cl in SMALL_STEM for dt in (FP32, BF16)], ids=_id)
def test_two_gradients_with_reduced_requires_grad(cuda, calls, op, shape, cl, dtype, req):
    c = _case(op, shape, True, op == "bn")
    got = _run(cuda, calls, c, dtype, cl, req=req)
    _check(got, _ref64(op, shape, True, op == "bn", "both"), cuda, dtype, req, f"{op} {shape} cl={cl} req={req}")


# ---- rounding of the two-gradient form (random normal data: the exact inputs cannot show a rounding) ------------------
def _close(a, b, rel, what):
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _randn_case(op, shape):
    g = torch.Generator().manual_seed(sum(shape) + (op == "stem"))
    C = shape[1]
    rn = lambda s: torch.randn(s, generator=g)
    oshape = _pooled(shape) if op == "stem" else shape
    return dict(weight=rn(C) * 0.5 + 1.0, bias=rn(C) * 0.3, mean=rn(C) * 0.4, var=torch.rand(C, generator=g) * 2 + 0.05,
                x=rn(shape), r=rn(shape) if op == "bn" else None, gy=rn(oshape), gy2=rn(oshape))


def _run_randn(dev, op, d, dtype, cl, grads, offset=()):
    """the fused op on random data: ``grads`` = (gy, gy2) through the two-output form, or (gy,) through the
    single-output form"""
    from handobjectconsist_amd.nn import frozen_bn

    bn = _module(dev, d["x"].shape[1], d["weight"], d["bias"], d["mean"], d["var"])
    # bf16-representable activations, so that an fp32 run is the bf16 run's "widened inputs"
    x = _put(d["x"].bfloat16(), dev, dtype, cl, "x" in offset).requires_grad_(True)
    r = _put(d["r"].bfloat16(), dev, dtype, cl, "r" in offset).requires_grad_(True) if d["r"] is not None else None
    dup = len(grads) == 2
    out = frozen_bn.bn_act(x, bn, residual=r, relu=True, dup=dup) if op == "bn" else frozen_bn.stem_pool(x, bn, dup=dup)
    ys = list(out) if dup else [out]
    torch.autograd.backward(ys, [_put(gr, dev, dtype, cl, f"gy{i + 1}" in offset) for i, gr in enumerate(grads)])
    return Ref(ys[0].detach(), x.grad, None if r is None else r.grad, bn.weight.grad, bn.bias.grad, None)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "cl"])
@pytest.mark.parametrize("shape", [(5, 16, 17, 30), (6, 64, 32, 32)], ids=_id)
@pytest.mark.parametrize("op", ["bn", "stem"])
def test_two_gradient_form_rounds_like_one_add(cuda, op, shape, cl, dtype):
    """fp32: kernel(gy, gy2) is bit-identical to the single-gradient kernel given gy + gy2 -- the same fp32 add, then
    the same kernel on the same values, channel sums included (fixed summation order).  bf16: the gradients are
    widened and added in fp32 and nothing is rounded before the store, so the outputs equal the fp32 kernel run on
    the widened inputs and gy.float() + gy2.float(), rounded once (the pattern of test_bn_act_bf16_activations, with
    its 1e-5 of scale for the parameter gradients)."""
    d = _randn_case(op, shape)
    gy, gy2 = d["gy"].to(cuda).bfloat16(), d["gy2"].to(cuda).bfloat16()   # bf16 values: the same data for both dtypes
    got = _run_randn(cuda, op, d, dtype, cl, (gy, gy2))
    ref = _run_randn(cuda, op, d, FP32, cl, (gy.float() + gy2.float(),))
    for field in ("y", "gx", "gr"):
        if getattr(ref, field) is not None:
            _same(getattr(got, field), getattr(ref, field).to(dtype), f"{op} {shape} {field}")
    if dtype == FP32:
        _same(got.gw, ref.gw, "grad weight")
        _same(got.gb, ref.gb, "grad bias")
    else:
        _close(got.gw, ref.gw, 1e-5, "grad weight")
        _close(got.gb, ref.gb, 1e-5, "grad bias")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_id)
@pytest.mark.parametrize("op,shape,which", [(op, s, w) for op, s in (("bn", (2, 8, 3, 5)), ("bn", (5, 16, 17, 30)),
                                                                     ("stem", (2, 4, 35, 70)), ("stem", (5, 16, 17, 30)))
                                            for w in ("gy2", "gy1", "x", "r") if not (op == "stem" and w == "r")], ids=_id)
def test_misaligned_channels_last_operand(cuda, op, shape, which, dtype):
    """A channels-last-contiguous operand whose storage starts 4 bytes (fp32) or 2 bytes (bf16) off the 16 / 8-byte
    boundary of a 4-element access -- a view into a larger buffer: the channels-last entry points refuse such a
    pointer (MR_ERR_BADARG), so the Python layer copies it to an aligned buffer first.  Same result as the aligned
    call, bit for bit."""
    d = _randn_case(op, shape)
    grads = (d["gy"], d["gy2"])
    got = _run_randn(cuda, op, d, dtype, True, grads, offset=(which,))
    ref = _run_randn(cuda, op, d, dtype, True, grads)
    assert got.y.is_contiguous(memory_format=torch.channels_last)
    for field in Ref._fields:
        if getattr(ref, field) is not None:
            _same(getattr(got, field), getattr(ref, field), f"{op} {shape} misaligned {which}: {field}")
