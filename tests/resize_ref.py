"""Pillow's ``Image.resize(size, Image.BILINEAR)`` for 8-bit RGB restated in numpy (a helper module: nothing pytest collects),
the contents generator and the geometry list tests/test_oracle_resize.py, tests/test_resize_host.py and
tests/test_gpu_resize.py share, and the fixture's reader.

The restatement follows ImagingResample (src/libImaging/Resample.c): per axis ``scale = in / out``, the triangle filter
stretched by ``max(scale, 1)``, taps ``lo .. lo + n - 1`` around ``(i + 0.5) * scale``, weights normalised in double and rounded
to 22-bit fixed point; the horizontal pass first, over the source rows the vertical taps span, an 8-bit intermediate image,
``clamp((2^21 + sum p k) >> 22, 0, 255)`` per pass; a pass only where its axis changes size.  All in IEEE double / int32 as
the C code has it; tests/test_oracle_resize.py holds it against the installed Pillow byte for byte."""
import hashlib
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_pil.npz")
PRECISION_BITS = 22
KINDS = ("uniform", "binary", "zeros", "full", "ramp_x", "ramp_y")


def taps_of(in_size, out_size):
    fs = max(in_size / out_size, 1.0)
    return 2 * int(math.ceil(1.0 * fs)) + 1


def tables(in_size, out_size):
    """(bounds int32 [out, 2] of (lo, n), coeffs int32 [out, taps], zero from n on) of one axis"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    taps = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, taps), np.int32)
    ss = 1.0 / fs
    for i in range(out_size):
        c = (i + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)  # (int(): towards zero, as the C cast)
        hi = min(int(c + support + 0.5), in_size)
        n = hi - lo
        w = []
        ww = 0.0
        for x in range(n):
            a = abs((x + lo - c + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            coeffs[i, x] = int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0)
        bounds[i] = lo, n
    return bounds, coeffs


def _pass(img, bounds, coeffs, axis):
    """one pass along ``axis`` (0: rows, 1: columns) of uint8 [..., H, W, 3] -> uint8 with that axis resized"""
    src = np.moveaxis(img.astype(np.int64), -3 + axis, 0)  # the resized axis first
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.int64)
    for i, (lo, n) in enumerate(bounds):
        k = coeffs[i, :n].astype(np.int64)
        out[i] = np.tensordot(k, src[lo:lo + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
    assert out.max(initial=0) < 2 ** 31 and out.min(initial=0) >= -2 ** 31, "the C code's 32-bit accumulator"
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, -3 + axis)


def resize(img, size):
    """uint8 [..., Hs, Ws, 3], size = (W, H) -> uint8 [..., H, W, 3]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    hs, ws = img.shape[-3:-1]
    w, h = int(size[0]), int(size[1])
    need_x, need_y = w != ws, h != hs
    if not need_x and not need_y:
        return img.copy()
    by, cy = tables(hs, h)
    if need_x:
        bx, cx = tables(ws, w)
        if need_y:  # the horizontal pass covers the rows the vertical taps span; the vertical bounds shift by the first
            first, last = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
            img = img[..., first:last, :, :]
            by = by - np.array([first, 0], np.int32)
        img = _pass(img, bx, cx, 1)
    if need_y:
        img = _pass(img, by, cy, 0)
    return img


def contents(kind, seed, width, height, frames=1):
    """uint8 [frames, height, width, 3] of one of ``KINDS`` (frames of a batch differ where the kind is random)"""
    rng = np.random.default_rng([seed, width, height])
    shape = (frames, height, width, 3)
    if kind == "uniform":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "full":
        return np.full(shape, 255, np.uint8)
    if kind in ("ramp_x", "ramp_y"):
        n = width if kind == "ramp_x" else height
        ramp = np.round(np.arange(n) * (255.0 / max(n - 1, 1))).astype(np.uint8)
        line = ramp[None, :, None] if kind == "ramp_x" else ramp[:, None, None]
        img = np.broadcast_to(line, (height, width, 3)).copy()
        img[..., 1] = 255 - img[..., 1]  # (the channels differ: ramp, 255 - ramp, ramp)
        return np.broadcast_to(img, shape).copy()
    raise ValueError(kind)


# ---- the geometries: (src_w, src_h, dst_w, dst_h) ----------------------------------------------------------------------------
SIDES = (1, 2, 3, 5, 8, 13, 16, 17, 31, 40)
HEIGHTS = ((7, 7), (9, 4), (4, 9), (33, 2))
NAMED = ((64, 36, 16, 9), (37, 23, 16, 9), (16, 9, 37, 23), (100, 50, 33, 50), (50, 100, 50, 33), (640, 480, 480, 270),
         (1920, 1080, 480, 270))
LARGE = (1920, 1080, 480, 270)  # the fixture holds the SHA-256 of Pillow's bytes only
RANDOM_KINDS = KINDS[:2]
HASH_ONLY_BYTES = 65536  # ... and of a random kind's output beyond this size (640 x 480 -> 480 x 270: it does not compress)


def hash_only(geom, kind):
    return geom == LARGE or (kind in RANDOM_KINDS and geom[2] * geom[3] * 3 > HASH_ONLY_BYTES)


def supported(geom):
    return taps_of(geom[0], geom[2]) <= 33 and taps_of(geom[1], geom[3]) <= 33


def sweep_geometries():
    """every pair of SIDES in width against HEIGHTS"""
    return [(ws, hs, w, h) for ws in SIDES for w in SIDES for hs, h in HEIGHTS]


def cases():
    """[(geometry, kind, seed)]: the sweep with a kind per case in turn (every kind meets every height pair and many width
    pairs), the named geometries with every kind; the large one with the two random kinds"""
    out = []
    for i, g in enumerate(sweep_geometries()):
        out.append((g, KINDS[(i // len(HEIGHTS) + i % len(HEIGHTS)) % len(KINDS)], 1000 + i))
    for j, g in enumerate(NAMED):
        for k, kind in enumerate(RANDOM_KINDS if g == LARGE else KINDS):
            out.append((g, kind, 5000 + 10 * j + k))
    return out


def case_key(geom, kind, seed):
    return "g%dx%d_%dx%d_%s_%d" % (*geom, kind, seed)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_fixture():
    """-> (meta: list of dicts with geometry / kind / seed / key, arrays): ``arrays[key]`` is Pillow's output (uint8 [H,W,3]),
    for the large geometry ``meta[i]["sha256"]`` instead"""
    z = np.load(GOLDEN)
    return json.loads(str(z["meta"]))["cases"], z
