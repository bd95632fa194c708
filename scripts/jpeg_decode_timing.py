"""The JPEG decode of one step's frames (192 files of 640 x 480, quality 90, gradient + noise) through the two-stage device
path and through Pillow on the host.
    python scripts/jpeg_decode_timing.py device [--frames 192] [--reps 10] [--threads 16] [--subsampling 2]
        jpegdecode.decode_batch: entropy decode in --threads threads, one upload, the two kernels; the wall time of the
        whole call (median of --reps) and of its host stage alone; for the kernels' own durations run it under
        ``rocprofv3 --kernel-trace --stats`` and read jpeg_idct_kernel / jpeg_color_kernel
    python scripts/jpeg_decode_timing.py host [--frames 192] [--workers 16] [--subsampling 2]
        Pillow's Image.open(...).convert("RGB") on the same files in --workers processes (no GPU is touched)
Each prints one JSON line."""
import argparse
import io
import json
import multiprocessing
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

H, W = 480, 640


def make_file(n, subsampling):
    from PIL import Image

    rng = np.random.default_rng(n)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (W + H - 2)], -1)
    frame = np.clip(base + rng.integers(-40, 41, base.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=90, subsampling=subsampling)
    return buf.getvalue()


def host_file(args):
    from PIL import Image

    data = make_file(*args)
    t0 = time.perf_counter()
    out = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return time.perf_counter() - t0, int(out[0, 0, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "host"))
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--subsampling", type=int, default=2, choices=(0, 1, 2))
    a = ap.parse_args()
    if a.mode == "host":
        with multiprocessing.get_context("spawn").Pool(a.workers) as pool:
            pool.map(host_file, [(n, a.subsampling) for n in range(a.workers)])  # (workers started, Pillow imported)
            per_file = [t for t, _ in pool.map(host_file, [(n, a.subsampling) for n in range(a.frames)], chunksize=1)]
        print(json.dumps({"mode": "host", "frames": a.frames, "workers": a.workers, "subsampling": a.subsampling,
                          "decode_ms_per_file_median": round(1e3 * float(np.median(per_file)), 2),
                          "decode_cpu_ms_total": round(1e3 * float(np.sum(per_file)), 1),
                          "decode_ms_per_step_at_workers": round(1e3 * float(np.sum(per_file)) / a.workers, 1)}))
    else:
        from concurrent.futures import ThreadPoolExecutor

        import torch

        from handobjectconsist_amd.datasets import jpegdecode

        dev = torch.device("cuda:0")
        files = [make_file(n, a.subsampling) for n in range(a.frames)]
        calls, stages = [], []
        for rep in range(a.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = jpegdecode.decode_batch(files, dev, threads=a.threads)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            with ThreadPoolExecutor(a.threads) as pool:
                packed = list(pool.map(jpegdecode.entropy_decode, files))
            t2 = time.perf_counter()
            if rep >= 2:
                calls.append(t1 - t0)
                stages.append(t2 - t1)
        print(json.dumps({"mode": "device", "frames": a.frames, "threads": a.threads, "subsampling": a.subsampling,
                          "call_ms_median": round(1e3 * float(np.median(calls)), 2), "call_ms_min": round(1e3 * float(np.min(calls)), 2),
                          "entropy_stage_ms_median": round(1e3 * float(np.median(stages)), 2),
                          "file_mb": round(sum(len(f) for f in files) / 1e6, 1), "packed_mb": round(sum(p.size for p in packed) / 1e6, 1),
                          "checksum": int(out.sum().item())}))


# (the workers are spawned: they import this module, so only the definitions above may run on import)
if __name__ == "__main__":
    main()
