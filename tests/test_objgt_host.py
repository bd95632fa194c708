"""datasets/objgt.py on the host (no device): the model bank's host functions, the packed rows, ``obj_geometry_host`` against
the float64 yardstick of tests/objgt_ref.py under its input-derived bound (K_ROUNDINGS = 9, counted there), and
``HandObjSet(obj_geometry=...)`` on ``SynthPoseDataset(obj_models=3)``: the host path against a direct ``pad_cyclic`` of the
accessors, the device path's samples with the same draws and every other key identical.  The entry points' refusals that
need no device are here too."""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests import objgt_ref as R

EXT = ["objverts3d", "objfaces", "objcanverts"]


def bank_and_models():
    from handobjectconsist_amd.datasets import objgt

    models = R.bank_models()
    return objgt.ObjectBank(models), models


def test_bank_host_functions_are_numpy_float32():
    bank, models = bank_and_models()
    assert len(bank) == 7 and bank.table().tolist()[:3] == [[0, 1, 0, 1], [1, 2, 1, 2], [3, 63, 3, 127]]
    for k, (v, f) in enumerate(models):
        box, centre, can = R.canonical(v)
        got_can, got_centre, got_scale = bank.canonical(k)
        assert got_can.dtype == np.float32 and np.array_equal(got_can.view(np.int32), can.view(np.int32)), k
        assert np.array_equal(got_centre.view(np.int32), centre.view(np.int32)) and np.array_equal(bank.box(k).view(np.int32), box.view(np.int32))
        assert got_scale == 1 and isinstance(got_scale, np.float32)
        assert bank.faces[k].dtype == np.int32 and np.array_equal(bank.faces[k], f)
    one = bank.canonical(0)  # a one-vertex model: its own centre, a zero canonical vertex
    assert np.array_equal(one[1], models[0][0][0]) and not one[0].any()
    # zeros of both signs: -0 is the minimum, +0 the maximum, whatever their order in the array
    for order in ([0.0, -0.0], [-0.0, 0.0]):
        v = np.array([[z, 1.0, -1.0] for z in order], np.float32)
        from handobjectconsist_amd.datasets import objgt

        box = objgt.ObjectBank([(v, [[0, 1, 0]])]).box(0)
        assert np.signbit(box[0]) and not np.signbit(box[3]) and box[0] == 0 and box[3] == 0


def test_bank_refusals():
    from handobjectconsist_amd.datasets import objgt

    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]])
    for bad_v, bad_f, match in ((np.zeros((0, 3)), f, "empty"), (v, np.zeros((0, 3), int), "empty"), (np.zeros((3, 2)), f, r"verts \[V,3\]"),
                                (v, np.array([[0, 1, 3]]), "face index"), (v, np.array([[0, -1, 2]]), "face index"),
                                (np.full((3, 3), np.nan), f, "not finite"), (v, np.zeros((2, 4), int), r"faces \[F,3\]")):
        with pytest.raises(ValueError, match=match):
            objgt.ObjectBank([(bad_v, bad_f)])
    bank = objgt.ObjectBank([(v, f)])
    with pytest.raises(ValueError, match="outside the bank"):
        objgt.obj_geometry_host(bank, [1], np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match="outside the bank"):
        objgt.frame_records(bank, [-1], np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match="pose must be"):
        objgt.obj_geometry_host(bank, [0], np.zeros((1, 4, 4)))
    with pytest.raises(ValueError, match="add up"):
        objgt.obj_geometry_host(bank, [0, 0], np.zeros((2, 3, 4)), groups=[1, 2])
    with pytest.raises(ValueError, match="GPU"):
        objgt.obj_geometry_batch(bank, [0], np.zeros((1, 3, 4)), device="cpu")
    with pytest.raises(ValueError, match="GPU"):
        bank.on("cpu")


def test_pack_unpack_round_trip_and_refusals():
    from handobjectconsist_amd.datasets import objgt

    rng = np.random.default_rng(3)
    pose = rng.standard_normal((4, 3, 4))
    rot = np.stack([R.rot_z(a) for a in (0.3, -2.0, 1.0, 0.0)])
    c3d = rng.standard_normal((4, 3)).astype(np.float32)
    rows = np.stack([objgt.pack_obj_info(k + 2, pose[k], flip=k % 2 == 1, rot_mat=rot[k], center3d=c3d[k]) for k in range(4)])
    assert rows.dtype == np.float32 and rows.shape == (4, objgt.OBJ_INFO_FLOATS)
    back = objgt.unpack_obj_info(rows)
    assert back["model"].tolist() == [2, 3, 4, 5] and back["flip"].tolist() == [False, True, False, True]
    assert np.array_equal(back["pose"], pose.astype(np.float32)) and np.array_equal(back["rot_mat"], rot) and np.array_equal(back["center3d"], c3d)
    plain = objgt.unpack_obj_info(objgt.pack_obj_info(0, pose[0])[None])
    assert plain["center3d"] is None and np.array_equal(plain["rot_mat"][0], np.eye(3)) and not plain["flip"][0]
    empty = objgt.unpack_obj_info(np.zeros((0, objgt.OBJ_INFO_FLOATS), np.float32))
    assert empty["model"].shape == (0,) and empty["center3d"] is None
    # the queried keys travel with the row: all five by default, the host path's keys for a partial query
    assert back["keys"] == objgt.KEYS and plain["keys"] == objgt.KEYS and empty["keys"] == objgt.KEYS
    for queries, keys in ((("frame", "objverts3d"), ("objverts3d",)), (("objfaces", "objverts3d"), ("objverts3d", "objfaces")),
                          (("objcanverts",), ("objcanverts", "objcantrans", "objcanscale"))):
        assert objgt.unpack_obj_info(objgt.pack_obj_info(0, pose[0], queries=queries)[None])["keys"] == keys
    with pytest.raises(ValueError, match="different queries, or for none"):
        objgt.unpack_obj_info(np.stack([rows[0], objgt.pack_obj_info(3, pose[1], center3d=c3d[1], queries=("objfaces",))]))
    with pytest.raises(ValueError, match="different queries, or for none"):
        objgt.unpack_obj_info(objgt.pack_obj_info(0, pose[0], queries=("frame",))[None])
    mixed = rows.copy()
    mixed[1] = objgt.pack_obj_info(3, pose[1])
    with pytest.raises(ValueError, match="some rows carry center3d"):
        objgt.unpack_obj_info(mixed)
    for bad in (rows[0], rows[:, :-1], rows[None]):
        with pytest.raises(ValueError, match="obj_info must be"):
            objgt.unpack_obj_info(bad)
    broken = rows.copy()
    broken[2, 0] = 1.5
    with pytest.raises(ValueError, match="model id"):
        objgt.unpack_obj_info(broken)
    broken[2, 0] = -1
    with pytest.raises(ValueError, match="model id"):
        objgt.unpack_obj_info(broken)
    for bad_id in (-1, 1 << 24):
        with pytest.raises(ValueError, match="model id"):
            objgt.pack_obj_info(bad_id, pose[0])
    with pytest.raises(ValueError, match="pose34"):
        objgt.pack_obj_info(0, np.eye(4))


@pytest.mark.parametrize("scale", [1.0, 1e-3], ids=["metres", "millimetres"])
@pytest.mark.parametrize("center", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("rot", [True, False], ids=["rotated", "unrotated"])
@pytest.mark.parametrize("flip", [True, False], ids=["mirrored", "unmirrored"])
def test_host_geometry_against_fp64(flip, rot, center, scale):
    """five frames in two dicts (models of 1, 65 and 257 vertices: two padded lengths): objverts3d within gamma_9 times the
    magnitudes of its terms, element by element; faces, padding pattern, centre and canonical vertices bit for bit"""
    from handobjectconsist_amd.datasets import objgt

    bank, models = bank_and_models()
    args = R.step_args(R.FIVE["model"], flip, rot, center, scale)
    got = objgt.obj_geometry_host(bank, groups=R.FIVE["groups"], **args)
    assert [g["objverts3d"].shape for g in got] == [(3, 65, 3), (2, 257, 3)] and [g["objfaces"].shape for g in got] == [(3, 129, 3), (2, 128, 3)]
    worst = R.check_step(f"host flip{flip} rot{rot} center{center} scale{scale}", got, R.step(models, groups=R.FIVE["groups"], **args))
    assert worst > 0.0  # (a bound that nothing comes near would check nothing; measured: about 0.1 - 0.3)
    # a single row repeated: every slot of the one-vertex model holds that vertex
    assert (got[0]["objverts3d"][0] == got[0]["objverts3d"][0][:1]).all() and (got[1]["objfaces"][1] == got[1]["objfaces"][1][:1]).all()


def test_host_geometry_from_the_rounded_rows_and_empty_steps():
    """through pack / unpack (the placement rounded once, then float32 all the way) the same bound holds against the float64
    placement; no frame at all gives empty arrays"""
    from handobjectconsist_amd.datasets import objgt

    bank, models = bank_and_models()
    args = R.step_args([6, 3, 1, 0], None, True, True, 1.0)
    rows = np.stack([objgt.pack_obj_info(args["model"][k], args["pose"][k], args["flip"][k], args["rot_mat"][k], args["center3d"][k]) for k in range(4)])
    got = objgt.obj_geometry_host(bank, **objgt.unpack_obj_info(rows))
    R.check_step("host, packed rows", got, R.step(models, groups=[4], **args))
    none = objgt.obj_geometry_host(bank, [], np.zeros((0, 3, 4)), groups=[0])
    assert none[0]["objverts3d"].shape == (0, 0, 3) and none[0]["objcanscale"].shape == (0,)
    rec, shapes, vrows, frows = objgt.frame_records(bank, **args, groups=[1, 3])
    ints = rec.view(np.int32)
    assert shapes == [(1, 1031, 2), (3, 64, 128)] and (vrows, frows) == (1031 + 3 * 64, 2 + 3 * 128)
    assert ints[:, 0].tolist() == [6, 3, 1, 0] and ints[:, 4].tolist() == [0, 1031, 1095, 1159] and ints[:, 5].tolist() == [0, 2, 130, 258]
    assert ints[:, 3].tolist() == [0, 1, 0, 1] and not ints[:, 6:8].any()
    assert np.array_equal(rec[1, 20:29].reshape(3, 3)[:, 0], -args["rot_mat"][1][:, 0])  # (the mirror folded: column 0 negated)


def _samples(geometry, seed=7, **kw):
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.utils import collate

    ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(96, 80), seed=2, sides=("right", "left"), obj_models=3)
    hs = handobjset.HandObjSet(ds, inp_res=(32, 32), sample_nb=2, sides="right", color_fn=None, obj_geometry=geometry, **kw)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    items = [hs[i] for i in (0, 3, 4)]
    state = (random.getstate(), np.random.get_state()[1].tolist(), torch.get_rng_state())
    return ds, hs, items, collate.seq_extend_collate(items, EXT), state


def test_synthetic_dataset_with_models():
    from handobjectconsist_amd.datasets import synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(96, 80), seed=2, obj_models=3)
    plain = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(96, 80), seed=2)
    assert [len(v) for v in ds.obj_bank.verts] == [20, 68, 146] and [len(f) for f in ds.obj_bank.faces] == [36, 132, 288]
    assert len({ds.get_obj_info(i)[0] for i in range(6)}) > 1, "the frames use more than one model"
    for i in range(6):  # the frames, intrinsics and hands do not move; None is the scene's object as ever
        assert np.array_equal(ds.get_image(i), plain.get_image(i)) and np.array_equal(ds.get_camintr(i), plain.get_camintr(i))
        assert np.array_equal(ds.get_hand_verts3d(i), plain.get_hand_verts3d(i))
        assert np.array_equal(plain.get_obj_verts_trans(i), plain.obj[i]) and plain.get_obj_faces(i) is plain.obj_faces
        model, pose = ds.get_obj_info(i)
        A, b = pose[:, :3], pose[:, 3]
        assert pose.dtype == np.float64 and np.allclose(A.dot(A.T), np.eye(3), atol=1e-12) and np.linalg.det(A) > 0
        assert np.abs(b - plain.obj[i].mean(0)).max() < 0.1
        ref, bound = R.frame(ds.obj_bank.verts[model], pose, False, None, None)
        assert (np.abs(ds.get_obj_verts_trans(i) - ref) <= bound).all()
        assert ds.get_obj_faces(i) is ds.obj_bank.faces[model]
    with pytest.raises(RuntimeError, match="no model ids"):
        plain.get_obj_info(0)
    given = synthpose.SynthPoseDataset(num_pairs=1, seed=2, obj_models=R.bank_models()[:2])
    assert [len(v) for v in given.obj_bank.verts] == [1, 2]


def test_handobjset_host_path_is_a_direct_pad_of_the_accessors():
    """obj_geometry="host" (the default): each collated dict's object arrays are the accessors' results, mirrored / rotated /
    centred by HandObjSet's own lines and padded with pad_cyclic; and obj_geometry_host, fed the device path's rows of the same
    seeds, gives the same bits"""
    from handobjectconsist_amd.datasets import objgt
    from handobjectconsist_amd.utils.collate import pad_cyclic

    ds, hs, items, batch, _ = _samples("host")
    assert hs.obj_geometry == "host"
    for pos, d in enumerate(batch):
        sams = [seq[pos] for seq in items]
        vmax, fmax = max(len(s["objverts3d"]) for s in sams), max(len(s["objfaces"]) for s in sams)
        assert len({len(s["objverts3d"]) for s in sams}) > 1 or pos, "models of different sizes meet in a dict"
        for k, s in enumerate(sams):
            assert np.array_equal(d["objverts3d"][k].numpy(), pad_cyclic(s["objverts3d"], vmax))
            assert np.array_equal(d["objfaces"][k].numpy(), pad_cyclic(s["objfaces"], fmax))
            assert np.array_equal(d["objcanverts"][k].numpy(), pad_cyclic(s["objcanverts"], vmax))
    # frame 0 of the first item, from the accessors by hand (frame 0 is a right hand: no mirror)
    s = items[0][0]
    rot = hs_rot(batch, items)
    pts = rot.dot(np.array(ds.get_obj_verts_trans(0), np.float32).T).T - s["center3d"]
    assert np.array_equal(s["objverts3d"], pts.astype(np.float32)) and np.array_equal(s["objcanverts"], ds.get_obj_verts_can(0)[0])
    _, _, _, dev_batch, _ = _samples("device")
    rows = [d["obj_info"].numpy() for d in dev_batch]
    res = objgt.obj_geometry_host(ds.obj_bank, groups=[len(r) for r in rows], **objgt.unpack_obj_info(np.concatenate(rows)))
    for d, r in zip(batch, res):
        for key in objgt.KEYS:
            want = d[key].numpy()
            assert np.array_equal(want.astype(r[key].dtype), r[key]) and want.shape == r[key].shape, key


def hs_rot(batch, items):
    """the augmentation rotation of the first item's first frame: ``__getitem__`` pops ``space_augm``, so it is drawn again by
    ``get_sample`` from the same seed"""
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(96, 80), seed=2, sides=("right", "left"), obj_models=3)
    hs = handobjset.HandObjSet(ds, inp_res=(32, 32), sample_nb=2, sides="right", color_fn=None)
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    rot = hs.get_sample(0)["space_augm"]["rot"]
    return np.array([[np.cos(rot), -np.sin(rot), 0], [np.sin(rot), np.cos(rot), 0], [0, 0, 1]]).astype(np.float32)


def test_handobjset_device_samples_carry_rows_and_nothing_else_moves():
    from handobjectconsist_amd.datasets import handobjset, objgt

    ds, _, _, host, host_state = _samples("host")
    _, hs, items, dev, dev_state = _samples("device")
    assert host_state[0] == dev_state[0] and host_state[1] == dev_state[1] and torch.equal(host_state[2], dev_state[2])
    gone = {"objverts3d", "objfaces", "objcanverts", "objcantrans", "objcanscale"}
    for a, b in zip(host, dev):
        assert set(a) - gone == set(b) - {"obj_info"} and not gone & set(b)
        assert b["obj_info"].shape == (3, objgt.OBJ_INFO_FLOATS) and b["obj_info"].dtype == torch.float32
        for key in set(a) - gone:
            same = torch.equal(a[key], b[key]) if torch.is_tensor(a[key]) else a[key] == b[key]
            assert same, key
        info = objgt.unpack_obj_info(b["obj_info"].numpy())
        assert np.array_equal(info["center3d"], a["center3d"].numpy()) and np.array_equal(info["flip"], a["flip"].numpy())
    with pytest.raises(ValueError, match="get_obj_info"):
        handobjset.HandObjSet(object(), obj_geometry="device")
    with pytest.raises(ValueError, match="obj_geometry must be"):
        handobjset.HandObjSet(ds, obj_geometry="gpu")
    # a partial query: the row asks for the keys the host sample holds
    for extra in (("objverts3d", "objfaces"), ("objcanverts",)):
        q = ("frame", "camintr", "joints3d", "side") + extra
        torch.manual_seed(11)  # (the same draws for both)
        host_s = handobjset.HandObjSet(ds, inp_res=(32, 32), color_fn=None, queries=q)[0]
        torch.manual_seed(11)
        dev_s = handobjset.HandObjSet(ds, inp_res=(32, 32), color_fn=None, queries=q, obj_geometry="device")[0]
        keys = objgt.unpack_obj_info(dev_s["obj_info"][None])["keys"]
        assert set(keys) == set(host_s) & set(objgt.KEYS) and set(host_s) - set(keys) == set(dev_s) - {"obj_info"}
        res = objgt.obj_geometry_host(ds.obj_bank, **objgt.unpack_obj_info(dev_s["obj_info"][None]))[0]
        assert set(res) == set(keys) and all(np.array_equal(res[k][0], np.asarray(host_s[k])) for k in keys)
    with pytest.raises(ValueError, match="keys must be among"):
        objgt.obj_geometry_host(ds.obj_bank, [0], np.zeros((1, 3, 4)), keys=("objverts2d",))
    # queries without an object: no row either
    hs2 = handobjset.HandObjSet(ds, inp_res=(32, 32), color_fn=None, obj_geometry="device", queries=("frame", "camintr", "joints3d", "side"))
    assert "obj_info" not in hs2[0]


def test_assemble_batch_refuses_before_any_upload(monkeypatch):
    """a mixed batch, a missing bank, an id outside the bank, an uncollated row: ValueError, and nothing has gone to a device
    (the device here does not exist: an upload would raise something else)"""
    from handobjectconsist_amd.datasets import handobjset, objgt

    ds, _, _, dev, _ = _samples("device")
    _, _, _, host, _ = _samples("host")
    moved = []
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: moved.append(a) or self)
    strip = lambda d: {k: v for k, v in d.items() if k not in ("frame", "affinetrans", "flip")}
    with pytest.raises(ValueError, match="mixes samples"):
        handobjset.assemble_batch([strip(dev[0]), strip(host[1])], "cuda", (32, 32), obj_bank=ds.obj_bank)
    with pytest.raises(ValueError, match="obj_bank"):
        handobjset.assemble_batch([strip(d) for d in dev], "cuda", (32, 32))
    small = objgt.ObjectBank(R.bank_models()[:1])
    with pytest.raises(ValueError, match="outside the bank"):
        handobjset.assemble_batch([strip(d) for d in dev], "cuda", (32, 32), obj_bank=small)
    with pytest.raises(ValueError, match="must be collated"):
        handobjset.assemble_batch(dict(strip(dev[0]), obj_info=dev[0]["obj_info"][0]), "cuda", (32, 32), obj_bank=ds.obj_bank)
    assert not moved


def test_entry_points_refuse_before_any_device_work():
    """MR_ERR_BADARG (-1) or MR_OK (0) with made-up pointers that are never dereferenced: no device needed"""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    null = ctypes.c_void_p(None)
    build = lambda **o: lib.mr_obj_bank_build(*[o.get(k, d) for k, d in (("verts", p), ("table", p), ("M", 3), ("V", 10), ("box", p), ("centre", p), ("can", p))], None)
    assert build(M=0) == 0 and build(M=0, verts=null, table=null, box=null, centre=null, can=null) == 0
    for bad in (dict(M=-1), dict(V=-1), dict(V=0), dict(verts=null), dict(table=null), dict(box=null), dict(centre=null), dict(can=null),
                dict(verts=ctypes.c_void_p(0x1002))):
        assert build(**bad) == -1, bad
    names = ("verts", "can", "centre", "faces", "table", "M", "V", "F", "frames", "N", "vrows", "frows", "o_verts", "o_can", "vcap", "o_faces", "fcap",
             "o_trans", "o_scale")
    valid = dict(M=3, V=10, F=12, N=2, vrows=20, frows=24, vcap=20, fcap=24)
    batch = lambda **o: lib.mr_obj_gt_batch(*[o.get(k, valid.get(k, p)) for k in names], None)
    assert batch(N=0, vrows=0, frows=0) == 0
    assert batch(N=0, vrows=0, frows=0, **{k: null for k in names if k not in valid}) == 0
    for bad in (dict(N=-1), dict(M=-1), dict(M=0), dict(V=0), dict(F=0), dict(vrows=-1), dict(frows=-1), dict(vcap=19), dict(fcap=23), dict(vcap=-1),
                dict(N=0), dict(vrows=1 << 31, vcap=1 << 32), dict(frows=1 << 31, fcap=1 << 32), dict(o_faces=ctypes.c_void_p(0x1004)),
                dict(frames=ctypes.c_void_p(0x1001)), *[{k: null} for k in names if k not in valid]):
        assert batch(**bad) == -1, bad
