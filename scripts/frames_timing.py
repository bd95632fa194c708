"""frames_to_batch at the shape of a step (3 x 64 frames of 640 x 480 -> 256 x 256, three mask channels) for every pair of
output types, with the sources warm in cache (back-to-back calls) and cold (a 1 GiB buffer is rewritten between calls),
medians over --reps calls.
    python scripts/frames_timing.py [--frames 192] [--reps 30]
prints one JSON line per pair of types: {"image", "mask", "warm_us", "cold_us", "out_mb"}.  The events bracket the whole
Python call -- the upload of the coefficients, the allocation of outputs and workspace, the table kernel and the streaming
kernel --, so these figures are those of the CALL, not of the ~100 us kernel.  For the kernel's own duration run the script
under ``rocprofv3 --kernel-trace`` and read the dispatches of ``frames_to_batch_kernel<IT, MT>``: per pair of types and
round they come as 2 x reps warm launches followed by reps cold ones."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from handobjectconsist_amd.datasets import frames as F
from handobjectconsist_amd.datasets import handutils

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=192)
ap.add_argument("--reps", type=int, default=30)
a = ap.parse_args()
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
res = (256, 256)
frames = torch.from_numpy(rng.integers(0, 256, (a.frames, 480, 640, 3), dtype=np.uint8)).to(dev)
coeffs = np.stack([handutils.pil_coeffs(handutils.get_affine_transform(rng.uniform((200, 150), (440, 330)), rng.uniform(150, 500), res,
                                                                       rot=0)[0]) for _ in range(a.frames)])
flush = torch.empty((1 << 28,), dtype=torch.float32, device=dev)


def timed(idt, mdt, cold):
    times = []
    for _ in range(a.reps):
        if cold:
            flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        img, mask = F.frames_to_batch(frames, coeffs, res, image_dtype=idt, mask_dtype=mdt)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times)), (img.numel() * img.element_size() + mask.numel() * mask.element_size()) / 1e6


for _ in range(2):  # (both orders: drift between the first and the last pair would show)
    for idt, mdt in ((torch.float32, torch.float32), (torch.bfloat16, torch.uint8), (torch.bfloat16, torch.float32),
                     (torch.float32, torch.uint8)):
        timed(idt, mdt, False)
        warm, mb = timed(idt, mdt, False)
        cold, _ = timed(idt, mdt, True)
        print(json.dumps({"image": str(idt), "mask": str(mdt), "warm_us": round(warm, 1), "cold_us": round(cold, 1), "out_mb": round(mb, 1)}))
