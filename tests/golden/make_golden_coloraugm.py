"""Generator of tests/golden/coloraugm_pil.npz: frames, colour plans, flip flags and what the installed Pillow makes of them
the way ``datasets/coloraugm.py``'s host path does (mirror if flipped, ``ImageFilter.GaussianBlur``, the ops in the plan's
order through ``ImageEnhance`` / the H-channel shift, mirror back).  Pillow only -- no kernel, no numpy restatement.

    python tests/golden/make_golden_coloraugm.py
"""
import json
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageFilter

BRIGHTNESS, SATURATION, HUE, CONTRAST = 1, 2, 3, 4  # MR_COLOR_OP_*
SIZES = [(1, 1), (5, 3), (7, 9), (37, 53), (48, 64)]  # (width, height)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "coloraugm_pil.npz")


def hue(img, factor):
    h, s, v = img.convert("HSV").split()
    np_h = ((np.array(h, dtype=np.int32) + int(factor * 255)) & 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def host_path(frame, radius, ops, flip):
    """``ops``: (code, factor) in application order; for hue the factor in [-0.5, 0.5]."""
    img = Image.fromarray(np.ascontiguousarray(frame[:, ::-1] if flip else frame)).filter(ImageFilter.GaussianBlur(radius))
    for code, f in ops:
        if code == HUE:
            img = hue(img, f)
        else:
            img = {BRIGHTNESS: ImageEnhance.Brightness, SATURATION: ImageEnhance.Color, CONTRAST: ImageEnhance.Contrast}[code](img).enhance(f)
    out = np.array(img)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def draw_case(rng, k):
    radius = [0.0, 0.3, 0.5, 1.0, 2.5, 6.0][k % 6] if k % 3 else float(np.float32(rng.uniform(0, 1.0)))
    codes = [int(c) for c in rng.permutation([BRIGHTNESS, SATURATION, HUE, CONTRAST])[: int(rng.integers(0, 5))]]
    # factors as float32 values: the plan stores them so, and Pillow's C receives a float
    ops = [(c, float(np.float32(rng.uniform(-0.15, 0.15) if c == HUE else rng.uniform(0.4, 1.6)))) for c in codes]
    return radius, ops


def plan_of(radius, ops):
    plan = np.zeros(9, np.float32)
    plan[0] = radius
    for k, (code, f) in enumerate(ops):
        plan[1 + k], plan[5 + k] = code, (int(f * 255) if code == HUE else f)
    return plan


def main():
    rng = np.random.default_rng(20)
    out, n = {}, 0
    for k in range(40):
        w, h = SIZES[k % len(SIZES)]
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 7 == 3:
            frame[:, : max(1, w // 2)] = (frame[:, : max(1, w // 2)] // 16) * 16  # flat patches: grey pixels, hue sectors
        radius, ops = draw_case(rng, k)
        flip = bool(k % 2)
        out[f"c{n}_in"], out[f"c{n}_plan"], out[f"c{n}_flip"] = frame[None], plan_of(radius, ops)[None], np.array([flip])
        out[f"c{n}_out"] = host_path(frame, radius, ops, flip)[None]
        n += 1
    # one batch of 6 frames of 33 x 70 (width x height), every frame its own plan, mixed flips
    frames = rng.integers(0, 256, (6, 70, 33, 3), dtype=np.uint8)
    cases = [draw_case(rng, 1 + k) for k in range(6)]
    cases[0] = (0.45, [(CONTRAST, 1.25), (HUE, 0.1), (BRIGHTNESS, 0.75), (SATURATION, 1.5)])
    cases[1] = (0.0, [])
    flips = np.array([0, 1, 1, 0, 1, 0], bool)
    out[f"c{n}_in"], out[f"c{n}_plan"], out[f"c{n}_flip"] = frames, np.stack([plan_of(*c) for c in cases]), flips
    out[f"c{n}_out"] = np.stack([host_path(f, r, ops, fl) for f, (r, ops), fl in zip(frames, cases, flips)])
    n += 1
    out["meta"] = np.array(json.dumps({"cases": n, "pillow": PIL.__version__}))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", n, "cases, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
