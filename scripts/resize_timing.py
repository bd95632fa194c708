"""Pillow's BILINEAR reduction of 1920 x 1080 frames to 480 x 270 (FPHAB's frames to the size the reference trains on) through
``frames.resize`` and through Pillow on the host.
    python scripts/resize_timing.py device [--frames 192] [--reps 10]
        ``frames.resize`` on --frames random frames resident on the GPU (192: 1.19 GB read, 75 MB written): device events
        around each of --reps calls, median and best, and the ratio to the HBM bound of those bytes at the 6.3 TB/s a
        streaming kernel achieves on an MI355X.  For the kernel's own duration run it under
        ``rocprofv3 --kernel-trace --stats`` in a run of its own and read frame_resize_kernel.
    python scripts/resize_timing.py host [--frames 4] [--reps 5]
        one core, no GPU: ``Image.resize((480, 270), Image.BILINEAR)`` per frame, the best of --reps passes over --frames
        frames
Each prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SRC, DST = (1920, 1080), (480, 270)
HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "host"))
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    a = ap.parse_args()
    if a.mode == "host":
        from PIL import Image

        frames, reps = a.frames or 4, a.reps or 5
        rng = np.random.default_rng(0)
        images = [Image.fromarray(rng.integers(0, 256, (SRC[1], SRC[0], 3), dtype=np.uint8)) for _ in range(frames)]
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            for im in images:
                im.resize(DST, Image.BILINEAR)
            best = min(best, (time.perf_counter() - t0) / frames)
        print(json.dumps({"mode": "host", "frames": frames, "reps": reps, "pillow_ms_per_frame": round(1e3 * best, 2)}))
        return
    import torch

    from handobjectconsist_amd.datasets import frames as F

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    n, reps = a.frames or 192, a.reps or 10
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (n, SRC[1], SRC[0], 3), dtype=torch.uint8, device=dev, generator=g)
    times = []
    for rep in range(reps + 2):  # (two warm-up calls: the tables are built in the first)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = F.resize(src, DST)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            times.append(e0.elapsed_time(e1))
    moved = src.numel() + out.numel()
    bound_ms = 1e3 * moved / HBM_BYTES_PER_S
    print(json.dumps({"mode": "device", "frames": n, "reps": reps, "read_mb": round(src.numel() / 1e6, 1),
                      "written_mb": round(out.numel() / 1e6, 1), "call_ms_median": round(float(np.median(times)), 3),
                      "call_ms_min": round(float(np.min(times)), 3), "hbm_bound_ms": round(bound_ms, 3),
                      "ratio_to_bound_min": round(float(np.min(times)) / bound_ms, 2), "checksum": int(out.sum().item())}))


if __name__ == "__main__":
    main()
