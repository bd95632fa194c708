"""The 2-D ground truth without a device (datasets/gt2d.py, datasets/handobjset.py's 2-D queries).

``points2d_host`` -- the host path and the device path's yardstick inside the product -- and BOTH of the reference's spellings of
the projection (ho3dv2.py:500-503; fhbhands.py:417-422, which multiplies the points by 1000 first) lie inside tests/gt2d_ref.py's
bound on every case of tests/gt2d_cases.py: the reference alone meets what the device is held to.  The transformed pixels are
within one ulp of the exact affine.  The info row and the records round-trip; every refusal of ``points2d_batch`` and of
``assemble_batch`` comes before anything touches a device (there is none here); ``HandObjSet``'s host path gives the keys, dtypes and
mirror of handobjset.py:160-225 without moving the random stream, and ``collate`` pads ``objverts2d`` with ``objverts3d``."""
import numpy as np
import pytest
import torch

from tests import gt2d_cases as C
from tests import gt2d_ref as R

case_ids = pytest.mark.parametrize("name", sorted(C.CASES))


@pytest.fixture(scope="module")
def models():
    return C.models()


@pytest.fixture(scope="module")
def bank(models):
    from handobjectconsist_amd.datasets import objgt

    return objgt.ObjectBank(models)


def bank_of(case, bank):
    return bank if "model" in case else None


# ---- values ----------------------------------------------------------------------------------------------------------------------
@case_ids
def test_host_path_is_inside_the_bound(models, bank, name):
    from handobjectconsist_amd.datasets import gt2d

    case = C.build(name)
    got = gt2d.points2d_host(bank=bank_of(case, bank), **C.call_args(case))
    R.check_step(f"host path, {name}", got, R.step(case, models), case["affine"], case["groups"], skip=case["skip"])
    for group, kind, frame, point in case["skip"]:  # numpy's own pattern: x = +h / 0, y = -h / 0, mirrored W - inf
        base = got[group][kind][frame, point]
        assert np.isinf(base).all() and base[1] < 0 and (base[0] < 0) == bool(case["flip"][sum(case["groups"][:group]) + frame])


def spellings(p32, K32):
    """the reference's two ways to the same pixel, on float32 points: ho3dv2.py's ``project`` and fhbhands.py's ``get_objverts2d``"""
    def project(points3d, cam_intr):
        hom_2d = np.array(cam_intr).dot(points3d.transpose()).transpose()
        return (hom_2d / hom_2d[:, 2:])[:, :2].astype(np.float32)
    return {"ho3d": project(p32, K32), "fphab": project(p32 * 1000, K32)}


@pytest.mark.parametrize("name", sorted(n for n, c in C.CASES.items() if "model" in c or "p3" in c))
def test_both_reference_spellings_are_inside_the_bound(models, name):
    """every case that projects, with float32 intrinsics (fhbhands.py:434-437 casts them) and, as the datasets hold them, float64 ones"""
    case = C.build(name)
    worst = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(sum(case["groups"])):
            sources = []
            if "model" in case:
                v, pose = models[case["model"][i]][0], case["pose"][i]
                sources.append(((pose[:, :3].dot(v.T).T + pose[:, 3]).astype(np.float32),) + R.bank_points(v, pose))
            if "points3d" in case:
                p = case["points3d"][i]
                sources.append((p, p.astype(np.float64), np.zeros(p.shape)))
            for p32, p64, e in sources:
                flip, W = bool(case["flip"][i]), case["width"][i]
                want, bound = R.base_ref(p64, e, case["camintr"][i], flip, W)
                ok = np.isfinite(want).all(1)
                assert ok.sum() >= len(ok) - len(case["skip"])
                for dt in (np.float32, np.float64):
                    for spelling, pts in spellings(p32, case["camintr"][i].astype(dt)).items():
                        if flip:
                            pts = pts.copy()
                            pts[:, 0] = int(W) - pts[:, 0]
                        assert pts.dtype == np.float32
                        ratio = float((np.abs(pts.astype(np.float64) - want)[ok] / bound[ok]).max())
                        key = f"{spelling}/{np.dtype(dt).name}"
                        worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"GT2D reference spellings, {name}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


def test_trans_is_the_hosts_own_arithmetic(bank):
    """``_trans`` of the host path is ``transform_coords`` of the base pixels, cast once"""
    from handobjectconsist_amd.datasets import gt2d, handutils

    case = C.build("mixed-three-dicts")
    got = gt2d.points2d_host(bank=bank, **C.call_args(case))
    lo = 0
    for g, d in zip(case["groups"], got):
        for kind in gt2d.KINDS:
            for i in range(g):
                M = np.concatenate([case["affine"][lo + i], [[0, 0, 1]]]).astype(np.float32)
                assert np.array_equal(d[kind + "_trans"][i], handutils.transform_coords(d[kind][i], M).astype(np.float32))
        lo += g
    assert [d["objverts2d"].shape[1] for d in got] == [986, 63, 40] and got[0]["handverts2d"].shape == (2, 778, 2)


# ---- packing -----------------------------------------------------------------------------------------------------------------------
def test_info_row_round_trips():
    from handobjectconsist_amd.datasets import gt2d

    rng = np.random.default_rng(3)
    K, M = rng.standard_normal((3, 3)).astype(np.float32), rng.standard_normal((3, 3)).astype(np.float32)
    rows = np.stack([gt2d.pack_gt2d_info(K, f, w, M, ("frame", "joints2d", "objverts2d_trans", "side")) for f, w in ((True, 640), (False, 272))])
    assert rows.shape == (2, gt2d.GT2D_INFO_FLOATS) and rows.dtype == np.float32
    back = gt2d.unpack_gt2d_info(rows)
    assert back["keys"] == ("objverts2d_trans", "joints2d") and back["flip"].tolist() == [True, False] and back["width"].tolist() == [640, 272]
    assert np.array_equal(back["camintr"], np.stack([K, K])) and np.array_equal(back["affine"], np.stack([M[:2], M[:2]]))
    for key in gt2d.KEYS:
        assert gt2d.unpack_gt2d_info(gt2d.pack_gt2d_info(K, False, 10, M, (key,))[None])["keys"] == (key,)
    with pytest.raises(ValueError, match="different queries"):
        gt2d.unpack_gt2d_info(np.stack([rows[0], gt2d.pack_gt2d_info(K, False, 640, M, ("joints2d",))]))
    with pytest.raises(ValueError, match="must be"):
        gt2d.unpack_gt2d_info(rows[:, :-1])
    with pytest.raises(ValueError, match="width"):
        gt2d.pack_gt2d_info(K, False, 0, M, ())
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        gt2d.pack_gt2d_info(K[:2], False, 5, M, ())


@case_ids
def test_records_round_trip(bank, name):
    """what ``point_records`` packs is what the kernel reads: modes, ascending rows without gaps, padded counts per dict and kind,
    the frames' own K / width / affine / placement"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import gt2d

    case = C.build(name)
    args = C.call_args(case)
    p3, p2 = args.pop("points3d", None), args.pop("points2d", None)
    rec, layout, rows = gt2d.point_records(bank=bank_of(case, bank), count3d=None if p3 is None else p3.shape[1], count2d=None if p2 is None else p2.shape[1], **args)
    f = gt2d.read_records(rec)
    assert rec.shape[1] == gt2d.RECORD_WORDS == 36 and rec.dtype == np.float32
    assert np.array_equal(f["row_offset"], np.concatenate([[0], np.cumsum(f["padded"])[:-1]])) and f["padded"].sum() == rows
    r, lo = 0, 0
    for g, blocks in zip(case["groups"], layout):
        for kind, frames, padded, first in blocks:
            sl, fr = slice(r, r + frames), slice(lo, lo + g)
            assert frames == g and f["row_offset"][r] == first and (f["padded"][sl] == padded).all()
            assert (f["mode"][sl] == {"objverts2d": _lib.GT2D_BANK, "handverts2d": _lib.GT2D_POINTS3D, "joints2d": _lib.GT2D_POINTS2D}[kind]).all()
            assert np.array_equal(f["camintr"][sl], case["camintr"][fr]) and np.array_equal(f["width"][sl], case["width"][fr])
            assert np.array_equal(f["affine"][sl], case["affine"][fr]) and np.array_equal(f["flip"][sl] != 0, case["flip"][fr])
            if kind == "objverts2d":
                counts = np.array([C.MODEL_V[m] for m in case["model"][fr]])
                assert np.array_equal(f["model"][sl], case["model"][fr]) and np.array_equal(f["pose"][sl], case["pose"][fr])
                assert np.array_equal(f["count"][sl], counts) and padded == counts.max()
            else:
                count = (p3 if kind == "handverts2d" else p2).shape[1]
                assert (f["count"][sl] == count).all() and padded == count and np.array_equal(f["src_first"][sl], np.arange(lo, lo + g) * count)
            r += frames
        lo += g
    assert r == len(rec)
    mirrored = gt2d.point_records(bank=bank_of(case, bank), count3d=None if p3 is None else p3.shape[1], count2d=None if p2 is None else p2.shape[1],
                                  points2d_mirrored=True, **args)[0]
    joints = f["mode"] == _lib.GT2D_POINTS2D
    assert not gt2d.read_records(mirrored)["flip"][joints].any() and np.array_equal(mirrored[~joints], rec[~joints])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_upload(bank, monkeypatch):
    """no device on this path: a refusal that came after an upload or a launch would fail differently"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import gt2d

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a launch"))
    case = C.call_args(C.build("mixed-three-dicts"))
    run = lambda **kw: gt2d.points2d_batch(bank=bank, device="cuda:0", **dict(case, **kw))
    with pytest.raises(ValueError, match="outside the bank"):
        run(model=np.array([5, 0, 2, 7, 1]))
    with pytest.raises(ValueError, match="outside the bank"):
        run(model=np.array([5, 0, -1, 6, 1]))
    with pytest.raises(ValueError, match="runs on a GPU"):
        gt2d.points2d_batch(bank=bank, device="cpu", **case)
    with pytest.raises(ValueError, match="share a device"):
        run(points3d=torch.from_numpy(case["points3d"]))
    with pytest.raises(ValueError, match="share a device"):
        run(points2d=torch.from_numpy(case["points2d"]))
    for bad, match in ((dict(pose=case["pose"][:4]), "pose must be"), (dict(model=case["model"][:4]), "model must be"), (dict(points3d=case["points3d"][:4]), "points3d must be"),
                       (dict(points2d=case["points2d"][..., :1]), "points2d must be"), (dict(points3d=case["points3d"][:, :0]), "points3d must be"),
                       (dict(camintr=case["camintr"][:, :2]), "camintr must be"), (dict(affine=case["affine"][:4]), "affine must be"), (dict(groups=[2, 2]), "do not add up"),
                       (dict(width=case["width"][:3]), "width must be"), (dict(width=0), "whole numbers"), (dict(flip=[True]), "flip must be"),
                       (dict(model=case["model"].astype(np.float32)), "integers"), (dict(pose=None), "together"), (dict(keys=("objverts3d",)), "keys must be")):
        with pytest.raises(ValueError, match=match):
            run(**bad)
    with pytest.raises(ValueError, match="together"):
        gt2d.points2d_batch(device="cuda:0", **case)  # no bank
    # more than 2^31 - 1 rows: three frames of 2^30 points each (the count alone is packed: nothing that large exists)
    with pytest.raises(ValueError, match="2\\^31 - 1 rows"):
        gt2d.point_records(case["camintr"][:3], None, 640, case["affine"][:3], count3d=1 << 30)
    assert gt2d.point_records(case["camintr"][:1], None, 640, case["affine"][:1], count3d=(1 << 31) - 1)[2] == (1 << 31) - 1


def test_no_frame_returns_empty_tensors_without_a_launch(bank, monkeypatch):
    """N == 0 on the host path; on the device path the same shapes come back without a launch (tests/test_gpu_gt2d.py)"""
    from handobjectconsist_amd.datasets import gt2d

    none = dict(camintr=np.zeros((0, 3, 3)), flip=None, width=640, affine=np.zeros((0, 2, 3)))
    got = gt2d.points2d_host(bank=bank, model=np.zeros(0, np.int64), pose=np.zeros((0, 3, 4)), points2d=np.zeros((0, 21, 2)), **none)
    assert got == [{}]
    rec, layout, rows = gt2d.point_records(bank=bank, model=np.zeros(0, np.int64), pose=np.zeros((0, 3, 4)), count2d=21, **none)
    assert rec.shape == (0, 36) and rows == 0 and [[b[:3] for b in blocks] for blocks in layout] == [[("objverts2d", 0, 0), ("joints2d", 0, 0)]]


# ---- the dataset's host path ---------------------------------------------------------------------------------------------------------
QUERIES_3D = ("frame", "camintr", "joints3d", "handverts3d", "objverts3d", "objfaces", "objcanverts", "side")
QUERIES_2D = ("affinetrans", "joints2d", "joints2d_trans", "objverts2d", "objverts2d_trans", "handverts2d", "handverts2d_trans")


def host_dataset(queries, **kw):
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(272, 248), seed=1, sides=("right", "left"), obj_models=3)
    return ds, handobjset.HandObjSet(ds, inp_res=(64, 64), sample_nb=2, sides="right", color_fn=None, queries=queries, **kw)


def test_host_queries_follow_the_reference_and_leave_the_random_stream_alone():
    from handobjectconsist_amd.datasets import handobjset, handutils

    assert not set(QUERIES_2D) & set(handobjset.DEFAULT_QUERIES)
    items, after = {}, {}
    for name, q in (("3d", QUERIES_3D), ("2d", QUERIES_3D + QUERIES_2D)):
        ds, hs = host_dataset(q)
        torch.manual_seed(5)
        items[name] = [hs[i] for i in (0, 3, 4)]
        after[name] = torch.rand(4)
    assert torch.equal(after["3d"], after["2d"]), "the 2-D queries move the random stream"
    mirrored = 0
    for idx, plain, seq in zip((0, 3, 4), items["3d"], items["2d"]):
        for pos, (a, b) in enumerate(zip(plain, seq)):
            i = idx ^ pos
            assert set(b) - set(a) == set(QUERIES_2D) - {"affinetrans"} and all(np.array_equal(a[k], b[k]) for k in a if k != "side")
            for kind, getter in (("joints2d", ds.get_joints2d), ("objverts2d", ds.get_objverts2d), ("handverts2d", ds.get_hand_verts2d)):
                want = getter(i).copy()
                if b["flip"]:
                    want[:, 0] = 272 - want[:, 0]
                    mirrored += 1
                assert b[kind].dtype == b[kind + "_trans"].dtype == np.float32 and np.array_equal(b[kind], want.astype(np.float32)), kind
                assert np.array_equal(b[kind + "_trans"], handutils.transform_coords(want, b["affinetrans"]).astype(np.float32)), kind
            assert b["joints2d"].shape == (21, 2) and b["handverts2d"].shape == (778, 2) and len(b["objverts2d"]) == len(b["objverts3d"])
    assert mirrored and mirrored < 18


def test_the_accessors_work_with_a_model_bank_and_without():
    from handobjectconsist_amd.datasets import synthpose

    for kw in (dict(), dict(obj_models=3)):
        ds = synthpose.SynthPoseDataset(num_pairs=2, seed=2, **kw)
        K = ds.get_camintr(1)
        for pts3d, pts2d in ((ds.get_joints3d(1), ds.get_joints2d(1)), (ds.get_obj_verts_trans(1), ds.get_objverts2d(1)), (ds.get_hand_verts3d(1), ds.get_hand_verts2d(1))):
            hom = np.asarray(K, np.float64).dot(np.asarray(pts3d, np.float64).T).T
            assert pts2d.dtype == np.float32 and pts2d.shape == (len(pts3d), 2) and np.allclose(pts2d, hom[:, :2] / hom[:, 2:], rtol=1e-5, atol=1e-3)


def test_collate_pads_objverts2d_with_objverts3d():
    from handobjectconsist_amd.utils import collate

    assert {"objverts2d", "objverts2d_trans", "objverts3d"} <= set(collate.EXTEND_QUERIES)
    ds, hs = host_dataset(QUERIES_3D + QUERIES_2D)
    torch.manual_seed(5)
    items = [hs[i] for i in (0, 3, 4)]
    assert len({len(it[0]["objverts2d"]) for it in items}) > 1
    for frame, d in enumerate(collate.seq_extend_collate(items, collate.EXTEND_QUERIES)):
        longest = max(len(it[frame]["objverts2d"]) for it in items)
        assert d["objverts2d"].shape == d["objverts2d_trans"].shape == (3, longest, 2) and d["objverts3d"].shape == (3, longest, 3)
        assert d["objverts2d"].dtype == torch.float32 and d["affinetrans"].shape == (3, 3, 3)
        for n, it in enumerate(items):
            v = len(it[frame]["objverts2d"])
            assert np.array_equal(d["objverts2d"][n].numpy(), it[frame]["objverts2d"][np.arange(longest) % v])


def test_construction_refusals():
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.models import synthnet

    class NoAccessors:
        def __init__(self, ds):
            self._ds = ds

        def __getattr__(self, name):
            if name in ("get_joints2d", "get_objverts2d", "get_hand_verts2d"):
                raise AttributeError(name)
            return getattr(self._ds, name)

        def __len__(self):
            return len(self._ds)

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    ds = synthpose.SynthPoseDataset(num_pairs=2, seed=1, obj_models=2, mano_layer=layer)
    make = lambda q, d=ds, **kw: handobjset.HandObjSet(d, queries=QUERIES_3D + q, **kw)
    for q, getter in ((("joints2d",), "get_joints2d"), (("objverts2d_trans",), "get_objverts2d"), (("handverts2d",), "get_hand_verts2d")):
        with pytest.raises(ValueError, match=getter):
            make(q, NoAccessors(ds))
    make((), NoAccessors(ds))  # (nothing asked: nothing needed)
    with pytest.raises(ValueError, match="points2d must be"):
        make((), points2d="gpu")
    with pytest.raises(ValueError, match="frame"):
        handobjset.HandObjSet(ds, queries=("side", "joints2d"))
    with pytest.raises(ValueError, match="obj_geometry"):
        make(("objverts2d",), points2d="device", hand_geometry="device")
    with pytest.raises(ValueError, match="hand_geometry"):
        make(("handverts2d_trans",), points2d="device", obj_geometry="device")
    with pytest.raises(ValueError, match="handverts3d"):
        handobjset.HandObjSet(ds, queries=("frame", "side", "handverts2d"), points2d="device", hand_geometry="device")
    with pytest.raises(ValueError, match="get_joints2d"):
        make(("joints2d",), NoAccessors(ds), points2d="device")
    make(("objverts2d", "handverts2d", "joints2d_trans"), points2d="device", obj_geometry="device", hand_geometry="device")


def test_device_samples_carry_rows_and_assemble_batch_refuses_before_any_upload(monkeypatch):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import gt2d, handobjset, synthpose
    from handobjectconsist_amd.models import synthnet
    from handobjectconsist_amd.utils import collate

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a launch"))
    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(272, 248), seed=1, sides=("right", "left"), obj_models=3, mano_layer=layer)
    kw = dict(inp_res=(64, 64), sample_nb=2, sides="right", color_fn=None, queries=QUERIES_3D + QUERIES_2D)
    host = handobjset.HandObjSet(ds, **kw)
    dev = handobjset.HandObjSet(ds, points2d="device", obj_geometry="device", hand_geometry="device", **kw)
    torch.manual_seed(9)
    a = [host[i] for i in (0, 3)]
    end = torch.rand(2)
    torch.manual_seed(9)
    b = [dev[i] for i in (0, 3)]
    assert torch.equal(end, torch.rand(2))
    for sa, sb in zip(a, b):
        for fa, fb in zip(sa, sb):
            assert not set(fb) & set(gt2d.KEYS) and fb["gt2d_info"].shape == (gt2d.GT2D_INFO_FLOATS,) and np.array_equal(fb["affinetrans"], fa["affinetrans"])
            assert fb["gt2d_joints"].dtype == np.float32 and np.array_equal(fb["gt2d_joints"], fa["joints2d"])
            info = gt2d.unpack_gt2d_info(fb["gt2d_info"][None])
            assert set(info["keys"]) == set(gt2d.KEYS) and info["width"][0] == 272 and bool(info["flip"][0]) == fb["flip"]
            assert np.array_equal(info["affine"][0], fa["affinetrans"][:2])
    batch = collate.seq_extend_collate(b, collate.EXTEND_QUERIES)
    hostb = collate.seq_extend_collate(a, collate.EXTEND_QUERIES)
    run = lambda dicts, **k: handobjset.assemble_batch(dicts, "cuda:0", (64, 64), **dict(dict(mano_layer=layer, obj_bank=ds.obj_bank), **k))
    with pytest.raises(ValueError, match="gt2d_info in 1 of 2"):
        run([batch[0], {k: v for k, v in batch[1].items() if k != "gt2d_info"}])
    with pytest.raises(ValueError, match="must be collated"):
        run([dict(batch[0], gt2d_info=batch[0]["gt2d_info"][0])])
    with pytest.raises(ValueError, match="needs assemble_batch\\(obj_bank"):
        run(batch, obj_bank=None)
    with pytest.raises(ValueError, match="asks for objverts2d"):
        run([{k: v for k, v in d.items() if k != "obj_info"} for d in batch])
    with pytest.raises(ValueError, match="asks for handverts2d"):
        run([{k: v for k, v in d.items() if k != "hand_info"} for d in batch])
    with pytest.raises(ValueError, match="asks for handverts2d"):
        run(batch, mano_layer=None)
    with pytest.raises(ValueError, match="asks for joints2d"):
        run([{k: v for k, v in d.items() if k != "gt2d_joints"} for d in batch])
    with pytest.raises(ValueError, match="different queries"):
        run([dict(batch[0], gt2d_info=torch.cat([batch[0]["gt2d_info"][:1], batch[0]["gt2d_info"][1:] * torch.tensor([1.0] * 17 + [0.5])]))])
    assert hostb[0]["joints2d"].shape == (2, 21, 2)
