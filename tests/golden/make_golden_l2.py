"""Generate tests/golden/warp_pair_consist_l2.npz and chain_metric_l2.npz by RUNNING THE REFERENCE'S OWN CODE on CPU with
``PyramidCriterion("l2")`` (torch.nn.MSELoss(reduction="none") + the per-sample masked mean, pyramidloss.py:56-62,
lossutils.py:1-8).

Build container only (needs /root/reference; import recipe and stubs: oracle/ref_glue.py, kornia stubbed there).  The
committed .npz files are data: seeded inputs and what the reference's code returned for them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_l2.py

warp_pair_consist_l2.npz  make_golden_warp.gen_pair_consist's inputs (same generators, same seed: a sample without a
                          valid pixel included) through the reference's ``pair_consist`` with the l2 criterion, both
                          values of ``use_backward``: losses, flow gradients, masks, warps, squared differences.
chain_metric_l2.npz       make_golden_trainer.gen_metric's warpbranch part (the METRIC workload's meshes at 256 x 256,
                          B = 2, trainer setting: gt_refs, first_only, use_backward) with the l2 criterion: loss,
                          ``diff_losses``, d loss / d predicted vertices of frame 0, flow samples; inputs as checksums.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_trainer as mgt  # noqa: E402  (installs the reference glue: oracle/ref_glue.py)
import make_golden_warp as mgw  # noqa: E402

ref = mgt.ref
T, N = mgt.T, mgt.N


def gen_pair_consist_l2():
    rng = np.random.default_rng(2)  # (make_golden_warp.gen_pair_consist's seed and draw order: the same inputs)
    B, H, W = 3, 19, 26
    crit = ref.pyramidloss.PyramidCriterion("l2")
    image_ref = rng.uniform(-0.5, 0.5, (B, 3, H, W)).astype(np.float32)
    image = rng.uniform(-0.5, 0.5, (B, 3, H, W)).astype(np.float32)
    jm_ref, jm = mgw.jitter(rng, B, H, W), mgw.jitter(rng, B, H, W)
    f12 = mgw.make_flows(rng, B, H, W, amp=1.5)
    f21 = mgw.make_flows(rng, B, H, W, amp=1.5)
    f12[2] = 0  # a sample with no valid pixel in either direction: the masked mean divides by 1
    f21[2] = 0
    gl = rng.uniform(0.5, 1.5, (B,)).astype(np.float32)
    res = dict(image_ref=image_ref, image=image, jitter_ref=jm_ref, jitter=jm, flow12=f12, flow21=f21, grad_loss=gl)
    for ub in (False, True):
        a, b = T(f12, True), T(f21, True)
        loss, masks, warps, diffs = ref.imgflowarp.pair_consist([a, b], T(image_ref), T(image), T(jm_ref), T(jm), crit,
                                                                use_backward=ub)
        (loss * T(gl)).sum().backward()
        tag = f"ub{int(ub)}"
        res[f"loss_{tag}"] = N(loss)
        res[f"grad_flow12_{tag}"] = N(a.grad) if a.grad is not None else np.zeros_like(f12)
        res[f"grad_flow21_{tag}"] = N(b.grad) if b.grad is not None else np.zeros_like(f21)
        if ub:
            for i in (0, 1):
                res[f"warp_mask{i + 1}"] = N(masks[i]["warp_mask"])
                res[f"full_mask{i + 1}"] = N(masks[i]["full_mask"])
                res[f"flow_mask{i + 1}"] = N(masks[i]["flow_mask"])
                res[f"warp{i + 1}"] = N(warps[i])
                res[f"diff{i + 1}"] = N(diffs[i])
    print("pair_consist l2: losses", res["loss_ub1"], "valid px", [int(res[f"full_mask{i}"].sum()) for i in (1, 2)])
    path = os.path.join(HERE, "warp_pair_consist_l2.npz")
    np.savez_compressed(path, **res)
    print(f"warp_pair_consist_l2.npz: {os.path.getsize(path) / 1024:.0f} KiB")


def gen_metric_l2():
    B, is_, seed = 2, 256, 4  # (make_golden_trainer.gen_metric's workload)
    TQ, BQ = ref.queries.TransQueries, ref.queries.BaseQueries
    s = mgt.synth.random_scene(B, seed=seed, image_size=is_)
    im_ref, im, jm_ref, jm = mgt.synth.random_images(B, is_, is_, seed)
    hand_faces, ignore = s["hand_faces"], mgt.synth.HAND_IGNORE_FACES
    arrays = {"checksum_" + k: np.array(np.asarray(v, np.float64).sum()) for k, v in
              dict(verts1=s["verts1"], verts2=s["verts2"], K1=s["K1"], faces=s["faces"], image0=im, image1=im_ref, jitter0=jm,
                   jitter1=jm_ref).items()}
    pred = [dict(hand=s["hand_verts1"], obj=s["obj_verts1"]), dict(hand=s["hand_verts2"] + 0.01, obj=s["obj_verts2"] - 0.01)]
    samples, results = [], []
    for k, (img, jit, K) in enumerate(((im, jm, s["K1"]), (im_ref, jm_ref, s["K2"]))):
        samples.append({TQ.IMAGE: T(img), TQ.JITTERMASK: T(jit), TQ.CAMINTR: T(K),
                        BQ.OBJFACES: T(s["obj_faces"][None].repeat(B, 0)), BQ.OBJVERTS3D: T(s["obj_verts" + "12"[k]]),
                        BQ.HANDVERTS3D: T(s["hand_verts" + "12"[k]])})
        results.append({"recov_handverts3d": T(pred[k]["hand"].astype(np.float32), True),
                        "recov_objverts3d": T(pred[k]["obj"].astype(np.float32), True)})
    arrays["pred1_hand"], arrays["pred1_obj"] = N(results[1]["recov_handverts3d"]), N(results[1]["recov_objverts3d"])
    loss, pair = ref.warpbranch.forward(samples, results, T(hand_faces)[None], mgt.training_renderer(is_), (is_, is_),
                                        ref.pyramidloss.PyramidCriterion("l2"), gt_refs=True, first_only=True,
                                        hand_ignore_faces=ignore, use_backward=True)
    loss.backward()
    arrays["wb_loss"], arrays["wb_diff_losses"] = N(loss), N(pair["diff_losses"])
    arrays["wb_grad_hand0"], arrays["wb_grad_obj0"] = N(results[0]["recov_handverts3d"].grad), N(results[0]["recov_objverts3d"].grad)
    assert results[1]["recov_handverts3d"].grad is None and results[1]["recov_objverts3d"].grad is None
    for d in (0, 1):
        mgt.flow_summary(arrays, f"wb_flow{d}", pair["recons_flows"][0][d], 210 + d, n=8000)
        arrays[f"wb_full_mask{d}_sum"] = np.array(float(pair["masks"][0][d]["full_mask"].sum()))
    print("warpbranch l2: loss", float(loss), "diff_losses", N(pair["diff_losses"]),
          "|g hand0|", float(results[0]["recov_handverts3d"].grad.abs().sum()))
    mgt.save("chain_metric_l2.npz", arrays, dict(batch=B, image_size=is_, scene_seed=seed, hand_ignore_faces=ignore,
                                                 criterion="l2", note="inputs = utils/synth.random_scene / random_images"))


if __name__ == "__main__":
    gen_pair_consist_l2()
    gen_metric_l2()
