"""The colour augmentation of one step's frames (192 frames of 640 x 480, blur radius 0.5 U(0, 1), all four ops in a random
order) on the GPU and on the host.
    python scripts/color_augm_timing.py device [--frames 192] [--reps 20]
        frames.color_augment, median of --reps calls bracketed by events (the CALL: plans, allocation, all launches); for the
        kernels' own durations run it under ``rocprofv3 --kernel-trace --stats`` and read the color_* kernels
    python scripts/color_augm_timing.py host [--frames 192] [--workers 16]
        datasets/coloraugm.py's Pillow path on the same frames and plans in --workers processes (no GPU is touched)
Each prints one JSON line."""
import argparse
import json
import multiprocessing
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from handobjectconsist_amd.datasets import coloraugm

H, W = 480, 640


def draw(n):
    """Frame n and its draws: (frame, blur radius, [(op, factor)] in application order)."""
    rng = np.random.default_rng(n)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    factors = {coloraugm.OP_BRIGHTNESS: rng.uniform(0.5, 1.5), coloraugm.OP_SATURATION: rng.uniform(0.5, 1.5),
               coloraugm.OP_HUE: rng.uniform(-0.15, 0.15), coloraugm.OP_CONTRAST: rng.uniform(0.5, 1.5)}
    return frame, 0.5 * rng.uniform(0, 1), [(int(c), float(factors[int(c)])) for c in rng.permutation(sorted(factors))]


def host_frame(n):
    from PIL import Image, ImageEnhance, ImageFilter

    frame, radius, ops = draw(n)
    t0 = time.perf_counter()
    img = Image.fromarray(frame).filter(ImageFilter.GaussianBlur(radius))
    for code, f in ops:
        if code == coloraugm.OP_HUE:
            img = coloraugm.adjust_hue(img, f)
        else:
            img = {coloraugm.OP_BRIGHTNESS: ImageEnhance.Brightness, coloraugm.OP_SATURATION: ImageEnhance.Color,
                   coloraugm.OP_CONTRAST: ImageEnhance.Contrast}[code](img).enhance(f)
    out = np.array(img)
    return time.perf_counter() - t0, int(out[0, 0, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "host"))
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    if a.mode == "host":
        with multiprocessing.get_context("spawn").Pool(a.workers) as pool:
            pool.map(host_frame, range(a.workers))  # (workers started, Pillow imported)
            t0 = time.perf_counter()
            per_frame = [t for t, _ in pool.map(host_frame, range(a.frames), chunksize=1)]
            wall = time.perf_counter() - t0  # (includes drawing the random frames: an upper bound of the augmentation's share)
        print(json.dumps({"mode": "host", "frames": a.frames, "workers": a.workers, "augment_ms_per_frame_median": round(1e3 * float(np.median(per_frame)), 2),
                          "augment_cpu_ms_total": round(1e3 * float(np.sum(per_frame)), 1),
                          "augment_ms_per_step_at_workers": round(1e3 * float(np.sum(per_frame)) / a.workers, 1), "wall_ms_with_frame_draws": round(1e3 * wall, 1)}))
    else:
        import torch

        from handobjectconsist_amd.datasets import frames as F

        dev = torch.device("cuda:0")
        drawn = [draw(n) for n in range(a.frames)]
        frames = torch.from_numpy(np.stack([d[0] for d in drawn])).to(dev)
        plans = np.zeros((a.frames, coloraugm.PLAN_LEN), np.float32)
        for n, (_, radius, ops) in enumerate(drawn):
            plans[n, 0] = radius
            for k, (code, f) in enumerate(ops):
                plans[n, 1 + k], plans[n, 5 + k] = code, (int(f * 255) if code == coloraugm.OP_HUE else f)
        times = []
        for rep in range(a.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = F.color_augment(frames, plans)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:
                times.append(e0.elapsed_time(e1) * 1e3)
        print(json.dumps({"mode": "device", "frames": a.frames, "call_us_median": round(float(np.median(times)), 1),
                          "call_us_min": round(float(np.min(times)), 1), "source_mb": round(frames.numel() / 1e6, 1),
                          "checksum": int(out.sum().item())}))


# (the workers are spawned: they import this module, so only the definitions above may run on import)
if __name__ == "__main__":
    main()
