"""numpy restatement of the colour augmentation of ``datasets/coloraugm.py`` -- Pillow's ``GaussianBlur``, the three
``ImageEnhance`` blends and the hue shift through HSV -- byte for byte, written from Pillow's published algorithms
(BoxBlur.c, Blend.c, Convert.c).  It is the checker of ``csrc/frame_color.hip``: tests/test_oracle_coloraugm.py pins it to
the installed Pillow, tests/test_gpu_coloraugm.py compares the kernels with it.  Test infrastructure: nothing in the
package imports it.

Widths matter and are spelled out: ``f32`` values are numpy float32 scalars / arrays (one IEEE operation per operator),
everything else is float64 or an integer type."""
import numpy as np

OP_NONE, OP_BRIGHTNESS, OP_SATURATION, OP_HUE, OP_CONTRAST = 0, 1, 2, 3, 4
f32 = np.float32


# ---- GaussianBlur = three box passes per axis (BoxBlur.c) ----
def box_radius(radius, passes=3):
    """_gaussian_blur_radius: the fractional box radius of one pass; float variables, the operations in float32."""
    r = f32(radius)
    s2 = r * r / f32(passes)
    L = np.sqrt(f32(12.0) * s2 + f32(1.0), dtype=f32)
    l = np.floor((L - f32(1.0)) / f32(2.0))  # noqa: E741
    a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * s2)
    a = a / (f32(6) * (s2 - (l + f32(1)) * (l + f32(1))))
    return f32(l + a)


def box_weights(fr):
    """(rad, ww, fw) of a pass: the integer radius, the 8.24 weight of a full tap and of the two fractional taps."""
    fr = f32(fr)
    rad = int(fr)
    ww = int(f32(1 << 24) / (fr * f32(2) + f32(1)))
    fw = ((1 << 24) - (rad * 2 + 1) * ww) // 2
    return rad, ww, fw


def box_pass(img, rad, ww, fw):
    """One pass along axis 1 of ``img`` [H, W, C] uint8 with edge clamping, rounded to uint8 (32-bit unsigned arithmetic)."""
    w = img.shape[1]
    src = img.astype(np.uint64)
    idx = np.arange(w)
    acc = np.zeros_like(src)
    for x in range(w):  # (taps beyond an edge all read the edge sample: counted, not walked)
        lo, hi = x - rad, x + rad
        clo, chi = max(lo, 0), min(hi, w - 1)
        acc[:, x] = src[:, clo:chi + 1].sum(1) + (clo - lo) * src[:, 0] + (hi - chi) * src[:, w - 1]
    far = src[:, np.clip(idx - rad - 1, 0, w - 1)] + src[:, np.clip(idx + rad + 1, 0, w - 1)]
    out = (acc * np.uint64(ww) + far * np.uint64(fw) + np.uint64(1 << 23))
    assert int(out.max(initial=0)) < (1 << 32)
    return (out >> np.uint64(24)).astype(np.uint8)


def gaussian_blur(img, radius):
    """``Image.filter(ImageFilter.GaussianBlur(radius))`` of an RGB frame [H, W, 3] uint8."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if radius == 0 or img.size == 0:
        return img.copy()
    rad, ww, fw = box_weights(box_radius(radius))
    out = img
    for _ in range(3):
        out = box_pass(out, rad, ww, fw)
    out = out.transpose(1, 0, 2)
    for _ in range(3):
        out = box_pass(out, rad, ww, fw)
    return np.ascontiguousarray(out.transpose(1, 0, 2))


# ---- ImageEnhance = blend(degenerate, image, factor) (Blend.c) ----
def luma(img):
    """convert("L"): ITU-R 601-2 in 16.16 fixed point."""
    v = img.astype(np.uint32)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, img, factor):
    factor = f32(factor)
    d = degenerate.astype(np.int32)
    t = d.astype(f32) + factor * (img.astype(np.int32) - d).astype(f32)  # float32: int + float * int
    if 0 <= factor <= 1:
        return t.astype(np.uint8)  # truncation; 0 <= t <= 255 by construction
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32)))  # (t is never NaN: the factor is finite)
    return out.astype(np.uint8)


def contrast_mean(img):
    """The grey level ImageEnhance.Contrast blends with: int(mean(L) + 0.5)."""
    lum = luma(img)
    return int(int(lum.sum(dtype=np.int64)) / lum.size + 0.5)


def enhance(img, op, factor):
    if op == OP_BRIGHTNESS:
        deg = np.zeros_like(img)
    elif op == OP_SATURATION:
        deg = np.repeat(luma(img)[..., None], 3, -1)
    elif op == OP_CONTRAST:
        deg = np.full_like(img, contrast_mean(img))
    else:
        raise ValueError(op)
    return blend(deg, img, factor)


# ---- hue shift through HSV (Convert.c rgb2hsv_row / hsv2rgb) ----
def rgb_to_hsv(img):
    """convert("HSV"): float variables mixed with double literals, as the C source has them."""
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = cr / maxc.astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    h_r = (bc - gc).astype(f32)  # float - float
    h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(f32)  # 2.0 + rc - bc: double, stored to a float
    h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(f32)
    h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)  # double expression, stored to a float
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((np.where(grey, 0, s).astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(hsv):
    """convert("RGB") of an HSV image: sector and remainder in double, the remainder and s / 255 stored to floats."""
    h, s, v = (hsv[..., k].astype(np.float64) for k in range(3))
    h6 = h * 6.0 / 255.0
    i = np.floor(h6).astype(np.int32)
    f = (h6 - i.astype(f32).astype(np.float64)).astype(f32).astype(np.float64)
    fs = (s / 255.0).astype(f32).astype(np.float64)
    p = np.clip(_round_half_away(v * (1.0 - fs)), 0, 255)
    q = np.clip(_round_half_away(v * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round_half_away(v * (1.0 - fs * (1.0 - f))), 0, 255)
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    sector = i % 6
    out = np.zeros(hsv.shape, np.float64)
    for k, chans in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(sector == k, chans[c], out[..., c])
    out = np.where((hsv[..., 1] == 0)[..., None], v[..., None], out)
    return out.astype(np.uint8)


def hue_shift_of(factor):
    """The integer the H byte moves by for a hue factor in [-0.5, 0.5]."""
    return int(factor * 255)


def adjust_hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


# ---- a whole plan ----
def apply_op(img, op, value):
    if op == OP_NONE:
        return img
    if op == OP_HUE:
        return adjust_hue(img, int(value))
    return enhance(img, op, value)


def apply_plan(frame, blur_radius, ops, flip=False):
    """``ops``: up to four (op code, value) in application order.  ``flip``: mirror, augment, mirror back."""
    img = np.ascontiguousarray(frame[:, ::-1] if flip else frame, dtype=np.uint8)
    img = gaussian_blur(img, blur_radius)
    for op, value in ops:
        if img.size:
            img = apply_op(img, int(op), value)
    return np.ascontiguousarray(img[:, ::-1] if flip else img)


def color_cube():
    """All 2^24 colours as a 4096 x 4096 RGB frame."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8)
