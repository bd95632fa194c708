"""Frame-pair scenes on meshes other than ``synth.random_scene``'s one (778 + 1002 vertices, 1552 + 2000 faces), and the table of
cases at which the pair step's launchers take each of their mesh-dependent decisions (a helper module: nothing pytest collects).

``mesh_scene`` returns what ``synth.random_scene`` returns -- the hand template plus a Fibonacci-sphere object of any vertex
count, shaped as ``synth.object_template`` shapes its sphere, cameras / poses / frame-2 motion sampled the same way -- with the
object's faces optionally padded by cyclic repetition (``collate.pad_cyclic``: face lists longer than 2 V, as real batches carry
them) or two object sizes in one batch, the smaller padded in vertices and faces to the larger (``collate.extend_collate``).

``CASES``: name -> shape + the decision the case exists for.  tests/test_pair_mesh_cases_host.py proves on the CPU, with
csrc/launch_plan.hpp itself, that each case reaches its decision on a 256-CU device; tests/test_gpu_pair_meshes.py runs them.
"""
import numpy as np

from handobjectconsist_amd.utils import collate, synth


def object_mesh(n_verts):
    """``synth.object_template`` at any vertex count: (verts [n,3] float32, faces [2n-4,3] int64); n = 0: an empty mesh."""
    if n_verts == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    v, f = synth.sphere_mesh(n_verts)
    v = np.sign(v) * np.abs(v) ** 0.6 * np.array([0.035, 0.06, 0.035], np.float32)
    return v.astype(np.float32), f


def mesh_scene(B, seed, image_size, obj_verts, obj_face_rows=None, mixed=None):
    """Two frames of a hand + object scene in camera coordinates, as ``synth.random_scene`` returns them (same keys; ``obj_faces``
    is [B,Fo,3] here, per sample).  ``obj_face_rows``: the object's faces padded cyclically to that many rows.  ``mixed``: the
    vertex count of a second, smaller object that the even samples carry, padded in vertices and faces to ``obj_verts``'s."""
    rng = np.random.default_rng(seed)
    hv, hf = synth.hand_template()
    ov, of = object_mesh(obj_verts)
    if obj_face_rows is not None:
        of = collate.pad_cyclic(of, obj_face_rows)
    Vo, Fo = ov.shape[0], of.shape[0]
    ovs, ofs = [ov] * B, [of] * B
    if mixed is not None:
        sv, sf = object_mesh(mixed)
        assert sv.shape[0] < Vo and obj_face_rows is None
        for b in range(0, B, 2):
            ovs[b], ofs[b] = collate.pad_cyclic(sv, Vo), collate.pad_cyclic(sf, Fo)
    ovs = np.stack(ovs).astype(np.float32)

    def place(template, rot, trans):  # (template [n,3] or [B,n,3])
        return (template @ np.transpose(rot, (0, 2, 1)) + trans[:, None]).astype(np.float32)

    # (the sampling order of synth.random_scene)
    scale = image_size / 256.0
    f = rng.uniform(300, 400, (B,)) * scale
    pp = (128 + rng.uniform(-8, 8, (B, 2))) * scale
    K = np.zeros((B, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f, f, pp[:, 0], pp[:, 1], 1
    rot_h = rng.normal(0, 1.0, (B, 3))
    rot_o = rng.normal(0, 1.0, (B, 3))
    t_h = np.stack([rng.uniform(-0.03, 0.03, B), rng.uniform(-0.03, 0.03, B), rng.uniform(0.35, 0.6, B)], 1)
    t_o = t_h + rng.uniform(-0.05, 0.05, (B, 3))
    hand1 = place(hv[None], synth._rodrigues(rot_h), t_h)
    obj1 = place(ovs, synth._rodrigues(rot_o), t_o)
    d = lambda s, n: rng.normal(0, s, (B, n))
    hand2 = place(hv[None], synth._rodrigues(rot_h + d(0.05, 3)), t_h + d(0.005, 3))
    obj2 = place(ovs, synth._rodrigues(rot_o + d(0.05, 3)), t_o + d(0.005, 3))
    obj_faces = np.stack(ofs).astype(np.int64) if B else np.zeros((0, Fo, 3), np.int64)
    faces = np.concatenate([hf[None].repeat(B, 0), obj_faces + synth.HAND_VERTS], 1)
    return {
        "verts1": np.concatenate([hand1, obj1], 1), "verts2": np.concatenate([hand2, obj2], 1),
        "hand_verts1": hand1, "hand_verts2": hand2, "obj_verts1": obj1, "obj_verts2": obj2,
        "hand_faces": hf, "obj_faces": obj_faces, "faces": faces, "K1": K, "K2": K.copy(),
    }


def camera(B, per_sample):
    """(R, t, dist_coeffs) as numpy: the identity camera with batch 1, or per sample small rotations about z, shifts and a little
    distortion (the values of test_gpu_warp.test_pair_step_equals_the_node_pair)"""
    if not per_sample:
        return np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), np.zeros((1, 5), np.float32)
    ang = np.linspace(-0.05, 0.05, B)
    R = np.eye(3)[None].repeat(B, 0)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    t = np.linspace(-0.01, 0.01, B)[:, None].repeat(3, 1)
    dist = np.linspace(-0.02, 0.02, B)[:, None] * np.array([1.0, 0.5, 0.1, -0.1, 0.2])
    return R.astype(np.float32), t.astype(np.float32), dist.astype(np.float32)


# PRO_* / form codes of csrc/launch_plan.hpp's BinPlan enums, as tests/host/launch_plan_cases.cpp prints them
PRO_NONE, PRO_IN_KERNEL, PRO_SEPARATE = 0, 1, 2
FACES_IN_KERNEL, FACES_LAUNCH = 0, 1
FORM_PLAIN, FORM_RECORDS, FORM_PROLOGUE = 0, 1, 2


def _case(B, raster, obj_verts, reach, obj_face_rows=None, mixed=None, crop=None, seed=0, jitter_channels=3, hand_batched=False,
          per_sample_cam=False, fused=True, node=False, note=""):
    """``reach``: field -> value of the line tests/host/launch_plan_cases.cpp prints for the case at 256 compute units"""
    return dict(B=B, raster=raster, obj_verts=obj_verts, obj_face_rows=obj_face_rows, mixed=mixed, crop=crop or (raster, raster), seed=seed,
                jitter_channels=jitter_channels, hand_batched=hand_batched, per_sample_cam=per_sample_cam, fused=fused, node=node,
                reach=reach, note=note)


# crop = (width, height).  Seeds are chosen so that the flows' non-zero pattern on the device equals the oracle's exactly (the
# precondition of the per-element gradient comparison); a case whose pattern differs FAILS, it is not skipped.
CASES = {
    "A": _case(1, 64, 4, dict(parts=8, two_launches=1, kh_raw=8, kh=7, least_obj_faces=4), seed=1, node=True,
               note="8 parts, count + fill launches, Kh 8 clamped to 7, an object part of 4 faces"),
    "B": _case(20, 64, 4, dict(parts=4, two_launches=0, kh_raw=4, kh=3), seed=2, note="4 parts in one launch, Kh 4 clamped to 3"),
    "C": _case(33, 64, 100, dict(parts=2, two_launches=0, kh_raw=2, kh=1), seed=3, note="2 parts, Kh 2 clamped to 1"),
    "D": _case(40, 64, 1002, dict(parts=2, kh_raw=0, kh=1, form=FORM_PROLOGUE, lds_opt_in=1), obj_face_rows=6000, seed=4,
               note="2 parts, Kh 0 clamped up to 1, PROLOGUE LDS above 48 KB"),
    "E": _case(2, 128, 1782, dict(parts=16, two_launches=1, colour_table=61440, colour_status=0), seed=5, node=True,
               note="16 parts, V = 2560: the colour-space table at its limit"),
    "F": _case(65, 32, 1782, dict(parts=1, sides="-1", form=FORM_PROLOGUE, lds_opt_in=1), seed=6,
               note="one part of a two-sided mesh (side -1), PROLOGUE LDS ~110 KB (opt-in)"),
    "G": _case(65, 32, 1002, dict(parts=1, lds_boxes=0, faces=FACES_LAUNCH, prologue=PRO_SEPARATE, form=FORM_PLAIN), obj_face_rows=9000, seed=7,
               note="boxes beyond LDS: lds_boxes 0, per-face launch, PRO_SEPARATE by plan"),
    "H": _case(2, 320, 333, dict(groups=16), crop=(200, 320), seed=8, node=True, note="V = 1111 (odd), 16 scatter groups, crop 200 x 320"),
    "I": _case(3, 96, 500, dict(), mixed=60, seed=9, note="the collate shape: two object sizes, the smaller padded cyclically"),
    "J": _case(4, 128, 300, dict(), seed=10, jitter_channels=1, hand_batched=True, per_sample_cam=True,
               note="batched hand faces, per-sample R / t / dist_coeffs, one-channel masks on another mesh"),
    "K": _case(2, 128, 1783, dict(colour_status=-2, scatter_status=0), seed=11, fused=False,
               note="V = 2561: flow_pair_loss returns None; composed path, gather fallback"),
    "L": _case(2, 64, 0, dict(), seed=12, fused=False, note="no object: the composed path on the hand alone"),
}
COMPACT_CASE, L2_CASE = "I", "J"  # one case also on the compact batch (bf16 images, u8 masks), one also with CRITERION_L2
# a shape an EXISTING test runs whose pair scatter takes 32 workgroups per image (test_gpu_compact_batch.SHAPES: 1 x 480)
EXISTING_480 = dict(B=1, raster=480, obj_verts=synth.OBJ_VERTS)


def plan_row(case):
    """the input row of tests/host/launch_plan_cases.cpp for a case: B2 V Fh Fo fill_back is"""
    Vo = case["obj_verts"]
    Fo = case.get("obj_face_rows") or max(2 * Vo - 4, 0)
    return (2 * case["B"], synth.HAND_VERTS + Vo, synth.HAND_FACES, Fo, 1, case["raster"])


def scene_of(case, seed=None):
    return mesh_scene(case["B"], case["seed"] if seed is None else seed, case["raster"], case["obj_verts"], case["obj_face_rows"], case["mixed"])
