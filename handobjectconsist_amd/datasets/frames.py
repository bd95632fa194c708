"""Decoded frames -> network-input batch on the GPU (``mr_frames_to_batch``): the device counterpart of
``transform_img`` + crop + ``to_tensor`` + ``normalize`` + jitter-mask generation that the reference runs
per sample in its DataLoader workers (meshreg/datasets/handobjset.py:361-379) -- and, in front of it, of the colour
augmentation of handobjset.py:339-358 (``mr_frames_color_augment``)."""
import numpy as np
import torch

from handobjectconsist_amd import _lib
from handobjectconsist_amd.datasets import handutils


def frames_to_batch(frames, affinetrans, inp_res, flip=None, mean=(0.5, 0.5, 0.5), std=(1.0, 1.0, 1.0),
                    jittermask=True, mask_channels=3, image_dtype=torch.float32, mask_dtype=torch.float32):
    """
    Args:
        frames: uint8 CUDA tensor [N, Hs, Ws, 3] -- the decoded (and colour-jittered) frames, HWC as PIL
            decodes them
        affinetrans: [N,3,3] source-pixel -> crop-pixel affines (``handutils.get_affine_transform``), numpy or
            tensor; or the ready Pillow coefficients [N,6] (float64)
        inp_res: (W, H) of the network input
        flip: optional [N] bools -- mirror the frame left-right first (handobjset.py:124-125)
        mean / std: ``normalize`` constants (the reference: 0.5 / 1 unless normalize_img)
        image_dtype: ``torch.float32`` (the default, the reference's batch format) or ``torch.bfloat16`` -- the fp32 value
            rounded to nearest-even, i.e. ``image_fp32.bfloat16()`` bit for bit
        mask_dtype: ``torch.float32`` or ``torch.uint8`` (1 where the fp32 mask is 1, else 0)
            (bfloat16 + uint8 is the COMPACT batch, DESIGN section 14: a third of the bytes, read as it is by the fused pair
            kernels and the bf16 trunk)

    Returns:
        image [N,3,H,W] of ``image_dtype``, jittermask [N,mask_channels,H,W] of ``mask_dtype`` in {0,1} (or None)
    """
    if image_dtype not in _lib.IMAGE_DTYPES:
        raise ValueError(f"image_dtype must be torch.float32 or torch.bfloat16, got {image_dtype!r}")
    if mask_dtype not in _lib.MASK_DTYPES:
        raise ValueError(f"mask_dtype must be torch.float32 or torch.uint8, got {mask_dtype!r}")
    _lib.check_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [N, Hs, Ws, 3]")
    frames = _lib.contig(frames, torch.uint8)
    N, Hs, Ws, _ = frames.shape
    W, H = int(inp_res[0]), int(inp_res[1])
    dev = frames.device
    aff = affinetrans.detach().cpu().numpy() if torch.is_tensor(affinetrans) else np.asarray(affinetrans)
    if aff.shape == (N, 3, 3):
        coeffs = np.stack([handutils.pil_coeffs(a) for a in aff]) if N else np.zeros((0, 6))
    elif aff.shape == (N, 6):
        coeffs = aff.astype(np.float64)
    else:
        raise ValueError("affinetrans must be [N,3,3] affines or [N,6] Pillow coefficients")
    coeffs_d = torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float64)).to(dev, non_blocking=True)
    flip_d = None
    if flip is not None:
        flip_d = torch.as_tensor(np.asarray(flip, dtype=np.uint8)).to(dev, non_blocking=True)
        if flip_d.shape != (N,):
            raise ValueError("flip must have one entry per frame")
    image = torch.empty((N, 3, H, W), dtype=image_dtype, device=dev)
    mask = torch.empty((N, mask_channels, H, W), dtype=mask_dtype, device=dev) if jittermask else None
    wbytes = int(_lib.load().mr_frames_to_batch_workspace_bytes(N, H, W))
    work = torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=dev)
    args = (_lib.ptr(frames), _lib.ptr(coeffs_d), _lib.ptr(flip_d), *[float(m) for m in mean], *[float(s) for s in std],
            _lib.ptr(work), wbytes, _lib.ptr(image), _lib.ptr(mask), int(mask_channels), N, Hs, Ws, H, W, _lib.stream_ptr(dev))
    if image_dtype == torch.float32 and mask_dtype == torch.float32:
        _lib.call("mr_frames_to_batch", *args)
    else:
        _lib.call("mr_frames_to_batch_typed", *args, _lib.DTYPE_CODES[image_dtype], _lib.DTYPE_CODES[mask_dtype])
    return image, mask


BILINEAR = 2  # Pillow's Image.BILINEAR: the one resampling filter ``resize`` offers
_RESIZE_TABLES = {}  # (Ws, Hs, W, H, device type, device index) -> the four device tables of that geometry


def resize_tables(in_size, out_size):
    """Pillow's coefficient tables of one axis (``mr_frames_resize_tables``; needs no device): (bounds int32 [out_size, 2] --
    per output index the first source index and the count of its taps --, coeffs int32 [out_size, taps], 22-bit fixed point,
    zero from the count on).  ValueError for a side below 1, NotImplementedError beyond 10752 pixels or a reduction by more
    than 16."""
    in_size, out_size = int(in_size), int(out_size)
    lib = _lib.load()
    taps = lib.mr_frames_resize_taps(in_size, out_size)
    if taps == -2:
        raise NotImplementedError(f"resize {in_size} -> {out_size}: sides run to {_lib.PNG_MAX_SIDE} pixels and a reduction to a "
                                  f"factor of 16 ({_lib.RESIZE_MAX_TAPS} taps)")
    if taps < 0:
        raise ValueError(f"resize {in_size} -> {out_size}: a side is below 1")
    bounds, coeffs = np.empty((out_size, 2), np.int32), np.empty((out_size, taps), np.int32)
    rc = lib.mr_frames_resize_tables(in_size, out_size, bounds.ctypes.data, coeffs.ctypes.data)
    if rc != taps:
        raise RuntimeError(f"mr_frames_resize_tables failed: {rc}")
    return bounds, coeffs


def _device_resize_tables(Ws, Hs, W, H, dev):
    dev = torch.device(dev)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (Ws, Hs, W, H, dev.type, index)  # (values only: a tensor or a device object never is a key)
    tabs = _RESIZE_TABLES.get(key)
    if tabs is None:
        host = resize_tables(Ws, W) + resize_tables(Hs, H)
        tabs = _RESIZE_TABLES[key] = tuple(torch.from_numpy(t).to(dev) for t in host)
    return tabs


def resize(frames, size, resample=BILINEAR):
    """Pillow's ``Image.resize(size, Image.BILINEAR)`` of a batch of decoded frames on the GPU, byte for byte
    (``mr_frames_resize``): one launch whatever N, on the caller's stream; not differentiable.

    Args:
        frames: uint8 CUDA tensor [N, Hs, Ws, 3]
        size: (W, H) of the result.  Sides run from 1 to 10752 pixels; enlargements of any factor, reductions up to a factor
            of 16 per axis -- beyond that NotImplementedError, from the sizes alone.
        resample: ``BILINEAR`` (Pillow's code 2) -- anything else is NotImplementedError; ``box`` and ``reducing_gap`` are
            not offered

    Returns:
        uint8 CUDA tensor [N, H, W, 3], a new tensor (a copy where the size is the frames' own).  The geometry's coefficient
        tables are built once per (Ws, Hs, W, H, device), uploaded and kept.
    """
    if resample != BILINEAR:
        raise NotImplementedError(f"resize: only BILINEAR (Pillow's filter code {BILINEAR}) is implemented, got {resample!r}")
    _lib.check_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [N, Hs, Ws, 3]")
    W, H = int(size[0]), int(size[1])
    N, Hs, Ws, _ = frames.shape
    if min(W, H, Ws, Hs) < 1:
        raise ValueError(f"resize {Ws} x {Hs} -> {W} x {H}: a side is below 1")
    frames = frames.detach()
    if (W, H) == (Ws, Hs):
        return frames.clone(memory_format=torch.contiguous_format)
    tabs = _device_resize_tables(Ws, Hs, W, H, frames.device)  # (refuses an unsupported geometry also where N = 0)
    frames = frames.contiguous()
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=frames.device)
    _lib.call("mr_frames_resize", _lib.ptr(frames), N, Ws, Hs, _lib.ptr(out), W, H, *[_lib.ptr(t) for t in tabs], None,
              _lib.stream_ptr(frames.device))
    return out


def color_augment(frames, plans, flip=None):
    """Gaussian blur + colour jitter of a batch of decoded frames on the GPU, byte for byte what ``coloraugm``'s host path
    (Pillow) gives for the same draws.

    Args:
        frames: uint8 CUDA tensor [N, Hs, Ws, 3]
        plans: [N, coloraugm.PLAN_LEN] plans of ``coloraugm.draw_color_plan`` (numpy or CPU tensor), one per frame
        flip: optional [N] bools -- the samples the host path mirrors around its augmentation (the result does not depend
            on them: every stage is mirror-symmetric)

    Returns:
        uint8 CUDA tensor [N, Hs, Ws, 3], a new tensor
    """
    _lib.check_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [N, Hs, Ws, 3]")
    frames = frames.contiguous()
    N, Hs, Ws, _ = frames.shape
    plans = np.ascontiguousarray(plans.detach().cpu().numpy() if torch.is_tensor(plans) else plans, dtype=np.float32)
    if plans.shape != (N, 9):
        raise ValueError("plans must hold one plan of 9 values per frame")
    radius = np.ascontiguousarray(plans[:, 0])
    if not np.all(np.abs(plans[:, 1:5]) <= 255) or np.any(plans[:, 1:5] != np.rint(plans[:, 1:5])):
        raise ValueError("plans: op codes must be integers (coloraugm.OP_*)")  # (the cast would truncate 1.5 to op 1)
    codes = np.ascontiguousarray(plans[:, 1:5]).astype(np.int32)
    values = np.ascontiguousarray(plans[:, 5:9])
    flip_h = None
    if flip is not None:
        flip_h = np.ascontiguousarray(np.asarray(flip, dtype=np.uint8))
        if flip_h.shape != (N,):
            raise ValueError("flip must have one entry per frame")
    out = torch.empty_like(frames)
    wbytes = int(_lib.load().mr_frames_color_augment_workspace_bytes(N, Hs, Ws))
    work = torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=frames.device)
    host = lambda a: None if a is None else a.ctypes.data  # noqa: E731  (host arrays: read before the call returns)
    _lib.call("mr_frames_color_augment", _lib.ptr(frames), _lib.ptr(out), host(flip_h), host(radius), host(codes), host(values),
              _lib.ptr(work), wbytes, N, Hs, Ws, _lib.stream_ptr(frames.device))
    return out
