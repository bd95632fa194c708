"""2-D ground truth of one step (B = 192 frames: the synthetic object models, 778 hand vertices, 21 joints), two ways:
    (a) the device path: gt2d.points2d_batch -- one upload of the records and the joints, one mr_gt2d_batch launch on the
        resident bank and on hand vertices that are already on the device; also the launch alone, on records that
        are already on the device; and, on its own line, the second MANO call that puts the camera-frame hand vertices there
        (gt2d.hand_cam_verts)
    (b) the host path it replaces: gt2d.points2d_host -- per frame the projection of the object's and the hand's vertices, the
        mirror, transform_coords, collate.pad_cyclic to the batch's longest model, np.stack -- and the upload of the six
        padded arrays, on one core (the hand's 3-D vertices are given: the MANO evaluation is neither path's here)
    python scripts/gt2d_timing.py [--batch 192] [--models 8] [--iters 200] [--windows 5] [--kernel-only]
Needs a GPU.  The two paths' results are compared first.  Device times: HIP events around ``--iters`` calls after a warm-up,
median and best of ``--windows`` windows.  Host times: a host clock around work that ends in a device synchronise, median of
``--windows``.  ``floor``: the bytes the launch must write and read (both outputs once, the hand vertices, joints and records
once; the bank is re-read from cache) over 8 TB/s.  ``--kernel-only``: the launch alone and nothing else (what a kernel trace of
this script should see).  Prints a small report."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch

    from handobjectconsist_amd.datasets import gt2d, handutils, objgt, synthpose
    from handobjectconsist_amd.models import synthnet

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    B = a.batch
    bank = objgt.ObjectBank(synthpose.procedural_models(a.models, seed=0))
    rng = np.random.default_rng(0)
    place = lambda: rng.standard_normal((B, 3, 1)) * [[0.08], [0.06], [0.1]] + [[0], [0], [0.6]]
    K = np.tile(np.array([[480.0, 0, 320.0], [0, 480.0, 240.0], [0, 0, 1]], np.float32), (B, 1, 1))
    affine = np.stack([handutils.get_affine_transform(rng.uniform(200, 440, 2), rng.uniform(150, 300), (256, 256), rot=rng.uniform(-np.pi, np.pi))[0]
                       for _ in range(B)])
    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    hand = dict(fullpose=(rng.standard_normal((B, 48)) * 0.2).astype(np.float32), shape=(rng.standard_normal((B, 10)) * 0.5).astype(np.float32),
                trans=place()[:, :, 0].astype(np.float32))
    cam_verts = gt2d.hand_cam_verts(layer, device=dev, **hand)
    frames = dict(camintr=K, flip=np.arange(B) % 2 == 1, width=640, affine=affine)
    args = dict(frames, bank=bank, model=rng.integers(0, len(bank), B), pose=np.concatenate([np.linalg.qr(rng.standard_normal((B, 3, 3)))[0], place()], 2).astype(np.float32),
                points2d=(rng.uniform(0, 1, (B, 21, 2)) * [640, 480]).astype(np.float32))
    host_verts = cam_verts.cpu().numpy()

    def device_call():
        return gt2d.points2d_batch(points3d=cam_verts, device=dev, **args)[0]

    def mano_call():
        return gt2d.hand_cam_verts(layer, device=dev, **hand)

    def host_one_core():
        got = gt2d.points2d_host(points3d=host_verts, **args)[0]
        t = {k: torch.from_numpy(v).to(dev, non_blocking=True) for k, v in got.items()}
        torch.cuda.synchronize()
        return t

    records, _, rows = gt2d.point_records(bank=bank, model=args["model"], pose=args["pose"], count3d=778, count2d=21, **frames)
    resident, joints, dbank = torch.from_numpy(records).to(dev), torch.from_numpy(args["points2d"]).to(dev), bank.on(dev)

    def launch_alone():
        return gt2d.run_records(resident, rows, dbank, cam_verts, joints)

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

    nv = [len(v) for v in bank.verts]
    byts = rows * 16 + B * 778 * 12 + B * 21 * 8 + records.nbytes
    print(f"gt2d_timing: B = {B} frames, {len(bank)} models of {min(nv)}..{max(nv)} vertices padded to {max(nv[m] for m in args['model'])} rows, 778 hand vertices, 21 joints: "
          f"{rows} rows, {len(records)} records")
    if a.kernel_only:
        med, best = events(launch_alone)
        print(f"  launch alone (records resident), events: median {med:.1f} us, best {best:.1f} us")
        return
    got, host = device_call(), host_one_core()
    torch.cuda.synchronize()
    for kind in gt2d.KINDS:
        print(f"  device vs host: {kind} max |diff| {float((got[kind] - host[kind]).abs().max()):.3g} px, {kind}_trans max |diff| "
              f"{float((got[kind + '_trans'] - host[kind + '_trans']).abs().max()):.3g} px")
    print(f"  bytes per step: {byts} written and read by the launch ({rows} rows x 16 B out, {B} x 778 x 12 B hand vertices, joints, records); "
          f"floor at 8 TB/s {byts / 8e12 * 1e6:.3f} us")
    print(f"  host path uploads {rows * 16} bytes per step, the device path {records.nbytes + args['points2d'].nbytes}")
    for name, fn, timer in (("device call (records packed and uploaded, one launch), events", device_call, events),
                            ("launch alone (records resident), events", launch_alone, events),
                            ("second MANO call (hand_cam_verts: upload + forward_full), events", mano_call, events),
                            ("host path, one core, to the end of the upload", host_one_core, clock)):
        med, best = timer(fn)
        print(f"  {name}: median {med:.1f} us, best {best:.1f} us")


if __name__ == "__main__":
    main()
