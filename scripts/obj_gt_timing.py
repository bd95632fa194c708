"""Ground-truth object meshes of one step (B = 192 frames, the synthetic models), two ways:
    (a) the device path: objgt.obj_geometry_batch -- one upload of the frame records, one mr_obj_gt_batch launch on the resident
        bank; also the launch alone, on records that are already on the device
    (b) the host path it replaces, as the default path runs it: per frame the numpy transform (A v + b, mirror, rotation,
        centre), the canonical copy and the faces, collate.pad_cyclic to the batch's longest model, np.stack, and the upload
        of the three padded arrays -- on one core, and split over 16 worker processes (the DataLoader's arrangement: the
        workers transform and pad, the parent stacks and uploads)
    python scripts/obj_gt_timing.py [--batch 192] [--models 8] [--iters 200] [--windows 5] [--workers 16]
Needs a GPU.  The two paths' results are compared first.  Device times: HIP events around ``--iters`` calls after a warm-up,
median and best of ``--windows`` windows.  Host times: a host clock around work that ends in a device synchronise, median of
``--windows``.  ``floor_us``: the bytes the launch must write and read (outputs once, records once; the bank is re-read from
cache) over 8 TB/s.  Prints a small report."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

_STATE = {}


def _host_frames(idx):
    """one worker's share: the frames' transformed, canonical and face arrays, padded to the batch's longest model"""
    from handobjectconsist_amd.utils.collate import pad_cyclic

    bank, a, vmax, fmax = _STATE["bank"], _STATE["args"], _STATE["vmax"], _STATE["fmax"]
    out = []
    for i in idx:
        m = a["model"][i]
        pts = np.array(bank.verts_trans(m, a["pose"][i]), dtype=np.float32)
        can = np.array(bank.canonical(m)[0], dtype=np.float32)
        if a["flip"][i]:
            pts[:, 0] = -pts[:, 0]
            can[:, 0] = -can[:, 0]
        pts = (a["rot_mat"][i].dot(pts.transpose(1, 0)).transpose() - a["center3d"][i]).astype(np.float32)
        out.append((pad_cyclic(pts, vmax), pad_cyclic(can, vmax), pad_cyclic(np.asarray(bank.faces[m], np.int64), fmax)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    from handobjectconsist_amd.datasets import objgt, synthpose

    B = a.batch
    bank = objgt.ObjectBank(synthpose.procedural_models(a.models, seed=0))
    rng = np.random.default_rng(0)
    ang = rng.uniform(-np.pi, np.pi, B)
    args = dict(model=rng.integers(0, len(bank), B), pose=np.concatenate([np.linalg.qr(rng.standard_normal((B, 3, 3)))[0], rng.standard_normal((B, 3, 1)) * 0.1], 2),
                flip=np.arange(B) % 2 == 1, center3d=(rng.standard_normal((B, 3)) * 0.1).astype(np.float32),
                rot_mat=np.stack([np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]]) for t in ang]).astype(np.float32))
    nv, nf = [len(v) for v in bank.verts], [len(f) for f in bank.faces]
    vmax, fmax = max(nv[m] for m in args["model"]), max(nf[m] for m in args["model"])
    _STATE.update(bank=bank, args=args, vmax=vmax, fmax=fmax)
    # the workers are forked before this process opens the GPU; they never touch it
    import multiprocessing

    pool = multiprocessing.get_context("fork").Pool(a.workers)
    shares = [list(range(k, B, a.workers)) for k in range(a.workers)]
    pool.map(_host_frames, shares)
    import torch

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")

    def upload(frames):
        t = [torch.from_numpy(np.stack([f[k] for f in frames])).to(dev, non_blocking=True) for k in range(3)]
        torch.cuda.synchronize()
        return t

    def host_one_core():
        return upload(_host_frames(range(B)))

    def host_workers():
        parts = pool.map(_host_frames, shares)
        frames = [None] * B
        for share, part in zip(shares, parts):
            for i, f in zip(share, part):
                frames[i] = f
        return upload(frames)

    def device_call():
        return objgt.obj_geometry_batch(bank, device=dev, **args)[0]

    records, _, vrows, frows = objgt.frame_records(bank, **args)
    resident = torch.from_numpy(records).to(dev)
    dbank = bank.on(dev)

    def launch_alone():
        return objgt.run_records(dbank, resident, vrows, frows)

    got, host = device_call(), host_one_core()
    torch.cuda.synchronize()
    same = [torch.equal(got["objcanverts"], host[1]), torch.equal(got["objfaces"], host[2])]
    diff = float((got["objverts3d"] - host[0]).abs().max())
    byts = 2 * vrows * 12 + frows * 24 + B * 16 + B * 128
    print(f"obj_gt_timing: B = {B} frames, {len(bank)} models of {min(nv)}..{max(nv)} vertices / {min(nf)}..{max(nf)} faces, padded to {vmax} / {fmax} rows")
    print(f"  device vs host: objcanverts equal {same[0]}, objfaces equal {same[1]}, objverts3d max |diff| {diff:.3g}")
    print(f"  bytes per step: {byts} written and read by the launch ({vrows} vertex rows x 2 x 12 B, {frows} face rows x 24 B, records); "
          f"floor at 8 TB/s {byts / 8e12 * 1e6:.3f} us")
    print(f"  host path uploads {B * (2 * vmax * 12 + fmax * 24)} bytes per step, the device path {records.nbytes}")

    def events(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / a.iters)
        return float(np.median(times)), min(times)

    def clock(fn):
        fn()
        times = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(times)), min(times)

    for name, fn, timer in (("device call (records packed and uploaded, one launch), events", device_call, events),
                            ("launch alone (records resident), events", launch_alone, events),
                            ("host path, one core, to the end of the upload", host_one_core, clock),
                            (f"host path, {a.workers} worker processes, to the end of the upload", host_workers, clock)):
        med, best = timer(fn)
        print(f"  {name}: median {med:.1f} us, best {best:.1f} us")
    pool.close()
    pool.join()


if __name__ == "__main__":
    main()
