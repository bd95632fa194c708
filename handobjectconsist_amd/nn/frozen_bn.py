"""BatchNorm2d with frozen statistics fused with the residual add and ReLU that follow it
(``mr_bn_act_forward`` / ``mr_bn_act_backward``; with a downsample branch's BatchNorm on top:
``mr_bn_add_bn_act_forward`` / ``_backward``).  The reference trains with ``--freeze_batchnorm``
(trainmeshwarp.py:205-206, 237-240): BatchNorm layers in eval mode, affine parameters trainable, so
``relu(bn(x))`` / ``relu(bn(x) + identity)`` / ``bn(x)`` of resnet.py:46-58 are per-channel affine maps."""
import torch
import torch.nn.functional as F

from handobjectconsist_amd import _lib


_ACT_DTYPES = {torch.float32: 0, torch.bfloat16: 1}  # act_dtype of the C-ABI


def _nhwc_channels_ok(C):
    return 4 <= C <= 1024 and 1024 % C == 0


def _layout(x):
    """(tensor in a layout the kernels take, channels_last flag): channels-last 4-D activations (what the trunk runs
    in, MIOpen's convolutions are faster there) stay as they are; everything else is made NCHW-contiguous."""
    if (x.dim() == 4 and _nhwc_channels_ok(x.shape[1]) and not x.is_contiguous()
            and x.is_contiguous(memory_format=torch.channels_last)):
        return x, 1
    return x.contiguous(), 0


def _aligned(t, cl):
    """``t`` itself, or -- for a channels-last operand whose storage does not start on the boundary of a 4-element
    access (16 bytes fp32, 8 bytes bf16: a view into a larger buffer) -- a copy that does.  The channels-last kernels
    have no scalar path and their entry points answer such a pointer with MR_ERR_BADARG; the NCHW kernels take their
    scalar path for it and need no copy."""
    if t is not None and cl and t.data_ptr() % (4 * t.element_size()):
        return t.clone(memory_format=torch.preserve_format)
    return t


def _channel_arrays(C, *tensors):
    """The per-channel operands as the kernels read them: fp32, contiguous, detached, each of shape [C]"""
    chan = [t.detach().float().contiguous() for t in tensors]
    if not all(t.shape == (C,) for t in chan):
        raise ValueError("channel arrays must be [C]")
    return chan


def _incoming(grad_y, grad_y2, dtype, cl):
    """The one or two gradients of a ``dup`` output as the backward kernels take them.  Arrival rule: with one consumer
    unused only one of the two arrives, and it goes first -- ``(g, None)``; ``(None, None)`` when neither did.  Each is
    cast to the activation type and brought to the forward's memory format and alignment."""
    if grad_y is None:
        grad_y, grad_y2 = grad_y2, None
    if grad_y is None:
        return None, None
    fmt = torch.channels_last if cl else torch.contiguous_format
    prep = lambda t: _aligned(t.to(dtype).contiguous(memory_format=fmt), cl)
    return prep(grad_y), (prep(grad_y2) if grad_y2 is not None else None)


def _workspace(sizer, dims, device, wanted):
    """(buffer for the partial sums of the parameter gradients or None when none is wanted, its size in bytes) from the
    entry point ``sizer`` (``mr_*_backward_workspace_bytes``)"""
    wbytes = int(getattr(_lib.load(), sizer)(*dims))
    return (torch.empty((wbytes,), dtype=torch.uint8, device=device) if wanted else None), wbytes


class _BnActFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, eps, relu, dup):
        ctx.set_materialize_grads(False)
        _lib.check_cuda(x, residual, weight, bias, running_mean, running_var)
        if x.dim() < 2 or x.dtype not in _ACT_DTYPES:
            raise ValueError("expected an fp32 or bf16 [N, C, ...] tensor")
        xc, cl = _layout(x)
        xc = _aligned(xc, cl)
        rc = None
        if residual is not None:
            if residual.shape != xc.shape or residual.dtype != xc.dtype:
                raise ValueError("residual must match x")
            rc = residual.contiguous(memory_format=torch.channels_last) if cl else residual.contiguous()
            rc = _aligned(rc, cl)
        N, C = xc.shape[:2]
        plane = xc[0, 0].numel() if N and C else 0
        w, b, m, v = _channel_arrays(C, weight, bias, running_mean, running_var)
        y = torch.empty_like(xc)
        _lib.call("mr_bn_act_forward", _lib.ptr(xc), _lib.ptr(rc), _lib.ptr(w), _lib.ptr(b), _lib.ptr(m), _lib.ptr(v),
                  float(eps), int(bool(relu)), _ACT_DTYPES[xc.dtype], cl, _lib.ptr(y), N, C, plane,
                  _lib.stream_ptr(xc.device))
        ctx.save_for_backward(xc, rc, w, b, m, v)
        ctx.cfg = (float(eps), bool(relu), N, C, plane, cl)
        # dup: the same activation as two autograd outputs (one per consumer); their gradients then arrive
        # separately and are summed inside the backward kernel instead of by a separate add pass
        return (y, y.view_as(y)) if dup else y

    @staticmethod
    def backward(ctx, grad_y, grad_y2=None):
        xc, rc, w, b, m, v = ctx.saved_tensors
        eps, relu, N, C, plane, cl = ctx.cfg
        need_x, need_r, need_w, need_b = ctx.needs_input_grad[:4]
        g, g2 = _incoming(grad_y, grad_y2, xc.dtype, cl)
        if g is None:
            return (None,) * 9
        dev = xc.device
        grad_x = torch.empty_like(xc)
        grad_r = torch.empty_like(xc) if (rc is not None and need_r) else None
        grad_w = torch.empty_like(w) if need_w else None
        grad_b = torch.empty_like(b) if need_b else None
        work, wbytes = _workspace("mr_bn_act_backward_workspace_bytes", (N, C), dev, need_w or need_b)
        _lib.call("mr_bn_act_backward", _lib.ptr(g), _lib.ptr(g2), _lib.ptr(xc), _lib.ptr(rc), _lib.ptr(w), _lib.ptr(b), _lib.ptr(m),
                  _lib.ptr(v), eps, int(relu), _ACT_DTYPES[xc.dtype], cl, _lib.ptr(grad_x), _lib.ptr(grad_r), _lib.ptr(grad_w),
                  _lib.ptr(grad_b),
                  _lib.ptr(work), wbytes, N, C, plane, _lib.stream_ptr(dev))
        return (grad_x if need_x else None), grad_r, grad_w, grad_b, None, None, None, None, None


def bn_act(x, bn, residual=None, relu=True, dup=False):
    """``relu(bn(x) [+ residual])`` for an ``nn.BatchNorm2d`` in eval mode (running statistics), one kernel.
    ``dup=True`` returns the result twice (two autograd outputs over one buffer) for an activation with two
    consumers -- a block's convolution and its identity branch -- whose gradients the backward kernel then sums."""
    if bn.training or not bn.track_running_stats:
        raise RuntimeError("bn_act needs frozen BatchNorm statistics (module.eval())")
    return _BnActFunction.apply(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu, dup)


class _BnAddBnActFunction(torch.autograd.Function):
    """relu(bn(x) + bn_d(xd)) on channels-last activations (``mr_bn_add_bn_act_forward`` / ``_backward``)"""

    @staticmethod
    def forward(ctx, x, xd, weight, bias, running_mean, running_var, eps, weight_d, bias_d, running_mean_d,
                running_var_d, eps_d, dup):
        ctx.set_materialize_grads(False)
        _lib.check_cuda(x, xd, weight, bias, running_mean, running_var, weight_d, bias_d, running_mean_d, running_var_d)
        xc, xdc = _aligned(x, 1), _aligned(xd, 1)
        N, C = xc.shape[:2]
        plane = xc[0, 0].numel() if N and C else 0
        chan = _channel_arrays(C, weight, bias, running_mean, running_var, weight_d, bias_d, running_mean_d, running_var_d)
        y = torch.empty_like(xc)
        _lib.call("mr_bn_add_bn_act_forward", _lib.ptr(xc), _lib.ptr(xdc), *[_lib.ptr(t) for t in chan[:4]], float(eps),
                  *[_lib.ptr(t) for t in chan[4:]], float(eps_d), _ACT_DTYPES[xc.dtype], _lib.ptr(y), N, C, plane,
                  _lib.stream_ptr(xc.device))
        ctx.save_for_backward(xc, xdc, *chan)
        ctx.cfg = (float(eps), float(eps_d), N, C, plane)
        return (y, y.view_as(y)) if dup else y

    @staticmethod
    def backward(ctx, grad_y, grad_y2=None):
        xc, xdc, *chan = ctx.saved_tensors
        eps, eps_d, N, C, plane = ctx.cfg
        need = ctx.needs_input_grad
        need_x, need_xd, need_w, need_b, need_wd, need_bd = need[0], need[1], need[2], need[3], need[7], need[8]
        g, g2 = _incoming(grad_y, grad_y2, xc.dtype, 1)
        if g is None:
            return (None,) * 13
        dev = xc.device
        grad_x, grad_xd = torch.empty_like(xc), torch.empty_like(xdc)
        grads = [torch.empty_like(chan[0]) if n else None for n in (need_w, need_b, need_wd, need_bd)]
        work, wbytes = _workspace("mr_bn_add_bn_act_backward_workspace_bytes", (N, C), dev, any(t is not None for t in grads))
        _lib.call("mr_bn_add_bn_act_backward", _lib.ptr(g), _lib.ptr(g2), _lib.ptr(xc), _lib.ptr(xdc),
                  *[_lib.ptr(t) for t in chan[:4]], eps, *[_lib.ptr(t) for t in chan[4:]], eps_d, _ACT_DTYPES[xc.dtype],
                  _lib.ptr(grad_x), _lib.ptr(grad_xd), *[_lib.ptr(t) for t in grads], _lib.ptr(work), wbytes, N, C, plane,
                  _lib.stream_ptr(dev))
        return ((grad_x if need_x else None), (grad_xd if need_xd else None), grads[0], grads[1], None, None, None,
                grads[2], grads[3], None, None, None, None)


def bn_add_bn_act(x, bn, xd, bn_d, dup=False):
    """``relu(bn(x) + bn_d(xd))`` for two ``nn.BatchNorm2d`` in eval mode: a residual block's tail with its downsample
    branch, one kernel each way instead of ``bn_act(xd, bn_d, relu=False)`` followed by ``bn_act(x, bn, residual=...)``
    -- the normalised downsample branch and its gradient are never written (``dup``: see ``bn_act``).  The fused kernels
    take channels-last activations; any other layout runs as those two ``bn_act`` calls."""
    for m in (bn, bn_d):
        if m.training or not m.track_running_stats:
            raise RuntimeError("bn_add_bn_act needs frozen BatchNorm statistics (module.eval())")
    if xd.shape != x.shape or xd.dtype != x.dtype:
        raise ValueError("xd must match x")
    if x.dim() < 2 or x.dtype not in _ACT_DTYPES:
        raise ValueError("expected fp32 or bf16 [N, C, ...] tensors")
    if _layout(x)[1] and _layout(xd)[1]:
        return _BnAddBnActFunction.apply(x, xd, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn_d.weight,
                                         bn_d.bias, bn_d.running_mean, bn_d.running_var, bn_d.eps, dup)
    return bn_act(x, bn, residual=bn_act(xd, bn_d, relu=False), dup=dup)


class _StemPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, dup):
        ctx.set_materialize_grads(False)
        _lib.check_cuda(x, weight, bias, running_mean, running_var)
        if x.dim() != 4 or x.dtype not in _ACT_DTYPES:
            raise ValueError("expected an fp32 or bf16 [N, C, H, W] tensor")
        xc, cl = _layout(x)
        xc = _aligned(xc, cl)
        N, C, H, W = xc.shape
        w, b, m, v = _channel_arrays(C, weight, bias, running_mean, running_var)
        oshape = (N, C, (H - 1) // 2 + 1 if H else 0, (W - 1) // 2 + 1 if W else 0)
        fmt = torch.channels_last if cl else torch.contiguous_format
        y = torch.empty(oshape, dtype=xc.dtype, device=xc.device, memory_format=fmt)
        # channels-last runs as layout 2, pooled records: the forward leaves every pooled value's arg-max position (1 byte)
        # and x - mean of that pixel (fp32) for the backward, which then needs neither x nor a pass over it
        layout = 2 if cl else 0
        records = None
        if cl:
            rbytes = int(_lib.load().mr_stem_pool_records_bytes(N, C, H, W))
            records = torch.empty((rbytes,), dtype=torch.uint8, device=xc.device)
        _lib.call("mr_stem_pool_forward", _lib.ptr(xc), _lib.ptr(w), _lib.ptr(b), _lib.ptr(m), _lib.ptr(v), float(eps),
                  _ACT_DTYPES[xc.dtype], layout, _lib.ptr(y), _lib.ptr(records), N, C, H, W, _lib.stream_ptr(xc.device))
        # NCHW: the backward recomputes bn(x) and needs x; layout 2: the records stand in for it
        ctx.save_for_backward(None if cl else xc, w, b, m, v, records)
        ctx.cfg = (float(eps), layout, tuple(xc.shape), xc.dtype, xc.device)
        return (y, y.view_as(y)) if dup else y

    @staticmethod
    def backward(ctx, grad_y, grad_y2=None):
        xc, w, b, m, v, records = ctx.saved_tensors
        eps, layout, shape, dtype, dev = ctx.cfg
        N, C, H, W = shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g, g2 = _incoming(grad_y, grad_y2, dtype, layout)
        if g is None:
            return (None,) * 7
        fmt = torch.channels_last if layout else torch.contiguous_format
        grad_x = torch.empty(shape, dtype=dtype, device=dev, memory_format=fmt)
        grad_w = torch.empty_like(w) if need_w else None
        grad_b = torch.empty_like(b) if need_b else None
        work, wbytes = _workspace("mr_stem_pool_backward_workspace_bytes", (N, C, H, W), dev, need_w or need_b)
        _lib.call("mr_stem_pool_backward", _lib.ptr(g), _lib.ptr(g2), _lib.ptr(xc), _lib.ptr(records), _lib.ptr(w), _lib.ptr(b),
                  _lib.ptr(m),
                  _lib.ptr(v), eps, _ACT_DTYPES[dtype], layout, _lib.ptr(grad_x), _lib.ptr(grad_w), _lib.ptr(grad_b),
                  _lib.ptr(work), wbytes, N, C, H, W,
                  _lib.stream_ptr(dev))
        return (grad_x if need_x else None), grad_w, grad_b, None, None, None, None


def stem_pool(x, bn, dup=False):
    """``MaxPool2d(3, 2, 1)(relu(bn(x)))`` for an ``nn.BatchNorm2d`` in eval mode: the ResNet stem, one kernel
    (``dup``: see ``bn_act``)."""
    if bn.training or not bn.track_running_stats:
        raise RuntimeError("stem_pool needs frozen BatchNorm statistics (module.eval())")
    return _StemPoolFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, dup)


class _ConvStemFunction(torch.autograd.Function):
    """The stem's convolution and ``stem_pool`` as one node for an image that wants no gradient: the backward forms the
    convolution's weight gradient straight from the pooled gradient and the records (``mr_stem_conv_wrw``) and the
    BatchNorm's from ``mr_stem_pool_param_grads``; the gradient of the convolution's output is never written."""

    @staticmethod
    def forward(ctx, image, conv_weight, weight, bias, running_mean, running_var, eps, dup):
        ctx.set_materialize_grads(False)
        _lib.check_cuda(image, conv_weight, weight, bias, running_mean, running_var)
        x = F.conv2d(image, conv_weight, None, 2, 3)  # the convolution of the composed path, not recorded
        x = _aligned(x.contiguous(memory_format=torch.channels_last), 1)
        N, C, H, W = x.shape
        w, b, m, v = _channel_arrays(C, weight, bias, running_mean, running_var)
        y = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last)
        records = torch.empty((int(_lib.load().mr_stem_pool_records_bytes(N, C, H, W)),), dtype=torch.uint8, device=x.device)
        _lib.call("mr_stem_pool_forward", _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(m), _lib.ptr(v), float(eps),
                  0, 2, _lib.ptr(y), _lib.ptr(records), N, C, H, W, _lib.stream_ptr(x.device))
        ctx.save_for_backward(image, w, b, m, v, records)
        ctx.cfg = (float(eps), (N, C, H, W), conv_weight.is_contiguous(memory_format=torch.channels_last), conv_weight.dtype)
        return (y, y.view_as(y)) if dup else y

    @staticmethod
    def backward(ctx, grad_y, grad_y2=None):
        image, w, b, m, v, records = ctx.saved_tensors
        eps, (N, C, H, W), w_cl, w_dtype = ctx.cfg
        _, need_cw, need_w, need_b = ctx.needs_input_grad[:4]
        g, g2 = _incoming(grad_y, grad_y2, torch.float32, 2)
        if g is None:
            return (None,) * 8
        dev = image.device
        lib = _lib.load()
        grad_cw = grad_w = grad_b = None
        if need_w or need_b:
            grad_w = torch.empty_like(w) if need_w else None
            grad_b = torch.empty_like(b) if need_b else None
            work, wbytes = _workspace("mr_stem_pool_backward_workspace_bytes", (N, C, H, W), dev, True)
            _lib.call("mr_stem_pool_param_grads", _lib.ptr(g), _lib.ptr(g2), _lib.ptr(records), _lib.ptr(w), _lib.ptr(b),
                      _lib.ptr(m), _lib.ptr(v), eps, 0, _lib.ptr(grad_w), _lib.ptr(grad_b), _lib.ptr(work), wbytes, N, C, H, W,
                      _lib.stream_ptr(dev))
        if need_cw:
            Hin, Win = image.shape[2:]
            grad_cw = torch.empty((C, 3, 7, 7), dtype=torch.float32, device=dev,
                                  memory_format=torch.channels_last if w_cl else torch.contiguous_format)
            work, wbytes = _workspace("mr_stem_conv_wrw_workspace_bytes", (N, C, Hin, Win), dev, True)
            _lib.call("mr_stem_conv_wrw", _lib.ptr(g), _lib.ptr(g2), _lib.ptr(records), _lib.ptr(w), _lib.ptr(b), _lib.ptr(m),
                      _lib.ptr(v), eps, _lib.ptr(image), _lib.ptr(grad_cw), int(w_cl), _lib.ptr(work), wbytes, N, C, Hin, Win,
                      3, 7, 2, 3, _lib.stream_ptr(dev))
        return None, grad_cw, grad_w, grad_b, None, None, None, None


def conv_stem_applies(image, conv, bn):
    """Does ``conv_stem_pool`` take this stem?  fp32 channels-last image that wants no gradient, no autocast, the ResNet
    stem's convolution (7 x 7, stride 2, padding 3, 3 -> 64 channels, no bias), frozen BatchNorm statistics."""
    w = conv.weight
    return (image.is_cuda and image.dim() == 4 and image.dtype == torch.float32 and not image.requires_grad
            and not torch.is_autocast_enabled("cuda")
            and image.numel() > 0 and image.is_contiguous(memory_format=torch.channels_last)
            and image.data_ptr() % 4 == 0
            and conv.kernel_size == (7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros" and conv.in_channels == 3
            and conv.out_channels == 64 and w.dtype == torch.float32
            and (w.is_contiguous(memory_format=torch.channels_last) or w.is_contiguous())
            and not bn.training and bn.track_running_stats and bn.weight.dtype == torch.float32)


def conv_stem_pool(image, conv, bn, dup=False):
    """``stem_pool(conv(image), bn)`` where ``conv_stem_applies``: the same values, and in the backward no gradient map of
    the convolution's output (``dup``: see ``bn_act``)."""
    if not conv_stem_applies(image, conv, bn):
        raise RuntimeError("conv_stem_pool does not take this stem (see conv_stem_applies)")
    return _ConvStemFunction.apply(image, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, dup)
