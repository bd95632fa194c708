"""The ground-truth hand meshes of one training step (192 frames by default) on the host, as the reference's DataLoader
workers produce them, and on the GPU in one call.
    python scripts/mano_gt_timing.py host [--frames 192] [--workers 16] [--reps 5]
        no GPU: ``manogt.hand_verts_host`` -- ``forward_torch`` at batch size 1 per sample, then the mirror / rotation / centre
        in numpy -- spread over --workers processes of one torch thread each (what DataLoader workers are); the wall time of
        all frames (median and best of --reps passes after a warm-up pass) and one worker's time per sample
    python scripts/mano_gt_timing.py device [--frames 192] [--reps 20]
        ``manogt.hand_verts_batch``: one upload of the stacked annotations, mr_mano_forward_full's three launches; the wall time
        of the whole call, synchronised (median and best of --reps after two warm-up calls).  For the kernels' own durations run
        it under ``rocprofv3 --kernel-trace --stats`` and read mano_pre_kernel / mano_blend_kernel / mano_skin_kernel.
Each prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def annotations(n, seed=0):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-np.pi, np.pi, n)
    return dict(fullpose=np.concatenate([rng.standard_normal((n, 3)), rng.standard_normal((n, 45)) * 0.3], 1).astype(np.float32),
                shape=rng.standard_normal((n, 10)).astype(np.float32),
                trans=(rng.standard_normal((n, 3)) * 0.1 + [0, 0, 0.5]).astype(np.float32),
                flip=np.arange(n) % 3 == 0,
                rot_mat=np.stack([np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) for a in ang]).astype(np.float32),
                center3d=(rng.standard_normal((n, 3)) * 0.05 + [0, 0, 0.5]).astype(np.float32))


_worker_layer = None


def _worker_init():
    global _worker_layer
    import torch

    from handobjectconsist_amd.models import synthnet

    torch.set_num_threads(1)
    _worker_layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)


def _worker_sample(args):
    from handobjectconsist_amd.datasets import manogt

    t0 = time.perf_counter()
    out = manogt.hand_verts_host(_worker_layer, **{k: v[None] for k, v in args.items()})
    return float(out.sum()), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "host"))
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=None)
    a = ap.parse_args()
    ann = annotations(a.frames)
    if a.mode == "host":
        import multiprocessing as mp

        samples = [{k: v[i] for k, v in ann.items()} for i in range(a.frames)]
        walls, per_sample = [], []
        with mp.get_context("spawn").Pool(a.workers, initializer=_worker_init) as pool:
            for rep in range((a.reps or 5) + 1):
                t0 = time.perf_counter()
                res = pool.map(_worker_sample, samples, chunksize=max(1, a.frames // (4 * a.workers)))
                if rep >= 1:
                    walls.append(time.perf_counter() - t0)
                    per_sample += [r[1] for r in res]
        print(json.dumps({"mode": "host", "frames": a.frames, "workers": a.workers, "reps": a.reps or 5,
                          "step_ms_median": round(1e3 * float(np.median(walls)), 2), "step_ms_min": round(1e3 * float(np.min(walls)), 2),
                          "sample_ms_median": round(1e3 * float(np.median(per_sample)), 3),
                          "checksum": round(sum(r[0] for r in res), 3)}))
    else:
        import torch

        from handobjectconsist_amd.datasets import manogt
        from handobjectconsist_amd.models import synthnet

        dev = torch.device("cuda:0")
        layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None).to(dev)
        calls = []
        for rep in range((a.reps or 20) + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = manogt.hand_verts_batch(layer, device=dev, **ann)
            torch.cuda.synchronize()
            if rep >= 2:
                calls.append(time.perf_counter() - t0)
        print(json.dumps({"mode": "device", "frames": a.frames, "reps": a.reps or 20,
                          "call_ms_median": round(1e3 * float(np.median(calls)), 3), "call_ms_min": round(1e3 * float(np.min(calls)), 3),
                          "checksum": round(float(out.double().sum().item()), 3)}))


if __name__ == "__main__":
    main()
