"""mr_gt2d_batch (csrc/gt2d/gt2d.hip) and the layers above it on a device: the 2-D ground truth -- projected, mirrored and cropped
points of the resident object bank, of the hand's camera-frame vertices and of the annotated joints.

Values, on every case of tests/gt2d_cases.py: the base pixels of BANK and POINTS3D records element by element against the float64
evaluation of the same formulas on the same float32 inputs under tests/gt2d_ref.py's bound (computed from the inputs: nothing is
taken from a run), those of POINTS2D records bit for bit, the transformed pixels within one ulp of the exact affine of the
device's own base pixels; the one point with hom_z == 0 gives numpy's inf / NaN pattern in its own two elements.  One mixed step
-- three dicts, all three kinds, one launch -- equals the separate calls bit for bit.  Output buffers are pre-filled with NaN and
are larger than the step: a slot nobody writes, or a write past the step's rows, fails.

Also: every case under the guard-band allocator, on strided / offset operands, on a side stream behind a delay
(tests/test_gpu_side_stream.py's arrangement) and under one graph capture replayed on changed records
(tests/test_gpu_graph_replay.py's recipe); the refusals, with the outputs untouched; ``HandObjSet(points2d="device")`` through
``assemble_batch`` against the same dataset with ``points2d="host"``; the metrics fed end to end.

Measured on an MI355X (``GT2D ...`` lines): largest base error / bound 0.33 over the step cases (0.05 to 0.33), 0.35 through the
dataset; metrics 8.793151 px (joints2d_base) and 8.793150 px (objverts2d_mepe) from both batches; side stream: largest
|side - default| 0 behind a 19.99 ms delay."""
import random

import numpy as np
import pytest
import torch

from tests import gt2d_cases as C
from tests import gt2d_ref as R

pytestmark = pytest.mark.gpu
case_ids = pytest.mark.parametrize("name", sorted(C.CASES))
NAMES = ["base", "trans"]


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def up(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)


@pytest.fixture(scope="module")
def models():
    return C.models()


@pytest.fixture(scope="module")
def bank(models):
    from handobjectconsist_amd.datasets import objgt

    return objgt.ObjectBank(models)


def bank_of(case, bank):
    return bank if "model" in case else None


def to_numpy(groups):
    return [{k: v.cpu().numpy() for k, v in g.items()} for g in groups]


def same_class(got, want):
    """float32 arrays: NaN where NaN, the same value (infinities with their sign) elsewhere"""
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ---- values --------------------------------------------------------------------------------------------------------------------
@case_ids
def test_step_against_fp64(cuda, models, bank, name):
    from handobjectconsist_amd.datasets import gt2d

    case = C.build(name)
    got = gt2d.points2d_batch(bank=bank_of(case, bank), device=cuda, **C.call_args(case))
    assert all(v.is_cuda and v.dtype == torch.float32 for g in got for v in g.values())
    host = to_numpy(got)
    R.check_step(f"device, {name}", host, R.step(case, models), case["affine"], case["groups"], skip=case["skip"])
    for group, kind, frame, point in case["skip"]:
        i = sum(case["groups"][:group]) + frame
        base = R.base_float32(case["points3d"][i][point:point + 1], case["camintr"][i], case["flip"][i], case["width"][i])
        assert not np.isfinite(base).any()
        assert same_class(host[group][kind][frame, point], base[0]), (host[group][kind][frame, point], base)
        assert same_class(host[group][kind + "_trans"][frame, point], R.trans_float64(base, case["affine"][i])[0])
    again = gt2d.points2d_batch(bank=bank_of(case, bank), device=cuda, **C.call_args(case))
    for a, b in zip(got, again):
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), f"two calls differ: {k}"
    # against the host path: both sides carry rounding, twice the bound; POINTS2D bit for bit
    ref = R.step(case, models)
    for d, h, r in zip(host, gt2d.points2d_host(bank=bank_of(case, bank), **C.call_args(case)), ref):
        for kind, (_, bound, exact) in r.items():
            with np.errstate(invalid="ignore"):
                err = np.abs(d[kind].astype(np.float64) - h[kind])
            ok = np.isfinite(bound) & np.isfinite(err)
            assert (err[ok] <= 2 * bound[ok]).all() and (not exact or np.array_equal(d[kind], h[kind])), kind


def test_mixed_step_equals_the_separate_calls(cuda, bank):
    """three dicts, all three kinds, one launch: the bits of a call per kind"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import gt2d

    case = C.call_args(C.build("mixed-three-dicts"))
    calls = []
    real = _lib.call
    _lib.call = lambda n, *a: (calls.append(n), real(n, *a))[1]
    try:
        bank.on(cuda)
        calls.clear()
        mixed = gt2d.points2d_batch(bank=bank, device=cuda, **case)
        assert calls == ["mr_gt2d_batch"], calls
    finally:
        _lib.call = real
    assert [sorted(d) for d in mixed] == [sorted(gt2d.KEYS)] * 3 and [tuple(d["objverts2d"].shape) for d in mixed] == [(2, 986, 2), (1, 63, 2), (2, 40, 2)]
    frames = {k: case[k] for k in ("camintr", "flip", "width", "affine", "groups")}
    for kind, source in (("objverts2d", dict(bank=bank, model=case["model"], pose=case["pose"])), ("handverts2d", dict(points3d=up(case["points3d"], cuda))),
                         ("joints2d", dict(points2d=case["points2d"]))):
        alone = gt2d.points2d_batch(device=cuda, **frames, **source)
        for d, a in zip(mixed, alone):
            assert sorted(a) == [kind, kind + "_trans"]
            for key in a:
                assert torch.equal(bits(d[key]), bits(a[key])), key
    only = gt2d.points2d_batch(bank=bank, device=cuda, keys=("joints2d_trans", "objverts2d"), **case)
    assert [sorted(d) for d in only] == [["joints2d_trans", "objverts2d"]] * 3 and torch.equal(only[2]["objverts2d"], mixed[2]["objverts2d"])


def test_no_frame_returns_empty_tensors_without_a_launch(cuda, bank, monkeypatch):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import gt2d

    bank.on(cuda)
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a launch"))
    got = gt2d.points2d_batch(np.zeros((0, 3, 3)), None, 640, np.zeros((0, 2, 3)), bank=bank, model=np.zeros(0, np.int64), pose=np.zeros((0, 3, 4)),
                              points3d=torch.zeros((0, 778, 3), device=cuda), points2d=np.zeros((0, 21, 2)), device=cuda)
    assert len(got) == 1 and sorted(got[0]) == sorted(gt2d.KEYS)
    assert all(v.is_cuda and v.dtype == torch.float32 and v.shape[0] == 0 and v.shape[2] == 2 for v in got[0].values())


# ---- the raw call ----------------------------------------------------------------------------------------------------------------
def step_inputs(cuda, bank, name, seed=0):
    """-> (the device tensors the call reads: records, then bank vertices and table, points3d, points2d where the case has
    them; which of them; rows)"""
    from handobjectconsist_amd.datasets import gt2d

    case = C.call_args(C.build(name, seed))
    p3, p2 = case.pop("points3d", None), case.pop("points2d", None)
    records, _, rows = gt2d.point_records(bank=bank_of(case, bank), count3d=None if p3 is None else p3.shape[1], count2d=None if p2 is None else p2.shape[1], **case)
    real, which = [up(records, cuda)], ["records"]
    if "model" in case:
        real += [up(np.concatenate(bank.verts), cuda), up(bank.table(), cuda)]
        which += ["verts", "table"]
    for key, pts in (("points3d", p3), ("points2d", p2)):
        if pts is not None:
            real.append(up(pts, cuda))
            which.append(key)
    return real, which, rows


def step_fn(which, rows):
    """the tensors of ``step_inputs`` -> one ``run_records`` call on the current stream: NAMES"""
    from handobjectconsist_amd.datasets import gt2d

    def fn(*tensors):
        t = dict(zip(which, tensors))
        return list(gt2d.run_records(t["records"], rows, {"verts": t["verts"], "table": t["table"]} if "verts" in t else None, t.get("points3d"), t.get("points2d")))
    return fn


def raw_step(cuda, tensors, which, rows, spare=300, capacity=None, **over):
    """mr_gt2d_batch as it is: outputs filled with NaN and ``spare`` rows longer than the step"""
    from handobjectconsist_amd import _lib

    t = dict(zip(which, tensors))
    nan = lambda: torch.full((max(rows, 0) + spare, 2), float("nan"), dtype=torch.float32, device=cuda)
    out = dict(base=nan(), trans=nan())
    P = _lib.ptr
    a = dict(verts=P(t.get("verts")), table=P(t.get("table")), M=t["table"].shape[0] if "table" in t else 0, V=t["verts"].shape[0] if "verts" in t else 0,
             p3=P(t.get("points3d")), rows3=t["points3d"].numel() // 3 if "points3d" in t else 0, p2=P(t.get("points2d")), rows2=t["points2d"].numel() // 2 if "points2d" in t else 0,
             records=P(t["records"]), N=t["records"].shape[0], rows=rows, base=P(out["base"]), trans=P(out["trans"]))
    a.update(over)
    rc = _lib.load().mr_gt2d_batch(a["verts"], a["table"], a["M"], a["V"], a["p3"], a["rows3"], a["p2"], a["rows2"], a["records"], a["N"], a["rows"], a["base"], a["trans"],
                                   rows + spare if capacity is None else capacity, _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    return rc, out


def test_every_slot_is_written_and_nothing_else(cuda, bank):
    from handobjectconsist_amd.datasets import gt2d

    real, which, rows = step_inputs(cuda, bank, "mixed-three-dicts")
    assert rows % 256 and rows > 256
    rc, out = raw_step(cuda, real, which, rows)
    assert rc == 0
    want = step_fn(which, rows)(*real)
    for key, w in zip(NAMES, want):
        body, tail = out[key][:rows], out[key][rows:]
        assert torch.equal(bits(body), bits(w)), f"{key}: the raw call and the layer differ"
        assert bool(torch.isnan(tail).all()), f"{key}: written past the step's rows"
        assert bool(torch.isfinite(body).all()), f"{key}: a slot nobody wrote"
    # a record whose padded length is shorter than its offsets say leaves the gap untouched; a wild model id, a wild block of a
    # dense array and a wild count are clamped to their buffers: every other row is written, finite, and nothing else is
    records = real[0].cpu().numpy().copy()
    f = {k: v.copy() for k, v in gt2d.read_records(records).items()}  # (the fields as they were: the edits below go to ``records``)
    ints = records.view(np.int32)
    banks = np.flatnonzero(f["mode"] == 0)
    bank_rec, hand_rec, joint_rec = int(banks[1]), int(np.flatnonzero(f["mode"] == 1)[0]), int(np.flatnonzero(f["mode"] == 2)[0])
    ints[bank_rec, 2], ints[banks[2], 5], ints[banks[3], 5] = 10, 1 << 30, -5
    ints[hand_rec, 6], ints[joint_rec, 6], ints[joint_rec, 3] = 1 << 30, -7, 1 << 29
    rc, gap = raw_step(cuda, [up(records, cuda)] + real[1:], which, rows)
    assert rc == 0
    lo, n = int(f["row_offset"][bank_rec]), int(f["padded"][bank_rec])
    assert n == 986
    for key in NAMES:
        assert bool(torch.isnan(gap[key][lo + 10:lo + n]).all()) and bool(torch.isnan(gap[key][rows:]).all())
        assert bool(torch.isfinite(gap[key][:lo + 10]).all()) and bool(torch.isfinite(gap[key][lo + n:rows]).all())
        assert torch.equal(bits(gap[key][:lo + 10]), bits(out[key][:lo + 10]))


def test_refusals_launch_nothing(cuda, bank):
    """null pointers, negative counts and a capacity too small: MR_ERR_BADARG, the outputs still NaN; the layer's own refusals"""
    from handobjectconsist_amd.datasets import gt2d

    real, which, rows = step_inputs(cuda, bank, "mixed-three-dicts")
    untouched = lambda out: all(bool(torch.isnan(t).all()) for t in out.values())
    for what, kw in (("capacity", dict(capacity=rows - 1)), ("negative capacity", dict(capacity=-1)), ("negative rows", dict(rows=-1)), ("negative records", dict(N=-1)),
                     ("negative models", dict(M=-1)), ("negative dense rows", dict(rows3=-1)), ("no records", dict(records=None)), ("no base", dict(base=None)),
                     ("no trans", dict(trans=None)), ("bank without vertices", dict(verts=None)), ("bank without table", dict(table=None)),
                     ("counted points3d missing", dict(p3=None)), ("counted points2d missing", dict(p2=None)), ("rows without records", dict(N=0))):
        rc, out = raw_step(cuda, real, which, kw.pop("rows", rows), **kw)
        assert rc == -1 and untouched(out), what
    rc, out = raw_step(cuda, real, which, 0, N=0)  # no record: nothing to do, nothing written
    assert rc == 0 and untouched(out)
    rc, out = raw_step(cuda, real, which, 0)  # records without rows
    assert rc == 0 and untouched(out)
    # a step whose source array is absent (the host refuses to pack it): the records' rows stay unwritten, the others are written
    rc, out = raw_step(cuda, real, which, rows, p2=None, rows2=0)
    f = gt2d.read_records(real[0].cpu().numpy())
    joints = np.zeros(rows, bool)
    for lo, n in zip(f["row_offset"][f["mode"] == 2], f["padded"][f["mode"] == 2]):
        joints[lo:lo + n] = True
    written = torch.isfinite(out["base"][:rows]).all(1).cpu().numpy()
    assert rc == 0 and np.array_equal(written, ~joints)
    case = C.call_args(C.build("mixed-three-dicts"))
    with pytest.raises(ValueError, match="outside the bank"):
        gt2d.points2d_batch(bank=bank, device=cuda, **dict(case, model=np.array([5, 0, 2, 7, 1])))
    with pytest.raises(ValueError, match="share a device"):
        gt2d.points2d_batch(bank=bank, device=cuda, **dict(case, points3d=torch.from_numpy(case["points3d"])))
    with pytest.raises(ValueError, match="records must be"):
        gt2d.run_records(real[0][:, :35], rows)
    with pytest.raises(TypeError):
        gt2d.run_records(real[0].cpu(), rows)


# ---- memory and streams ------------------------------------------------------------------------------------------------------------
@case_ids
def test_guard_bands(cuda, monkeypatch, bank, name):
    """the step with every tensor inside guard bands: no band changes, every pointer the entry point gets lies in a guarded
    interior, and the values are those of the plain run"""
    from handobjectconsist_amd import _lib
    from tests import guarded_alloc as G

    real, which, rows = step_inputs(cuda, bank, name)
    fn = step_fn(which, rows)
    plain = fn(*real)
    torch.cuda.synchronize()
    alloc = G.GuardedAllocator(cuda)
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append((n, a)), real_call(n, *a))[1])
    alloc.install(monkeypatch)
    try:
        got = fn(*[alloc.guard(t) for t in real])
        damage = alloc.check()
    finally:
        alloc.uninstall()
        monkeypatch.setattr(_lib, "call", real_call)
    strangers = alloc.pointer_report(calls)
    print(f"GT2D guard bands {name}: {alloc.count()} guarded allocations, {alloc.pointers_seen} pointer arguments")
    assert not damage, "\n".join(damage)
    assert not strangers, strangers
    assert [n for n, _ in calls] == ["mr_gt2d_batch"] and alloc.pointers_seen == len(real) + 2
    for key, a, b in zip(NAMES, got, plain):
        assert alloc.holds(a), f"{key}: not in guarded storage"
        assert torch.equal(bits(a), bits(b)), key


def strided(t):
    """a [rows, columns] float tensor's values as a column slice of a wider one, behind a storage offset"""
    wide = torch.full((t.shape[0] + 2, t.shape[1] + 5), float("nan"), dtype=t.dtype, device=t.device)
    wide[1:-1, 3:3 + t.shape[1]] = t
    return wide[1:-1, 3:3 + t.shape[1]]


@case_ids
def test_strided_operands_are_made_dense(cuda, bank, name):
    """records, vertices and the dense points as column slices of wider tensors behind a storage offset, a transposed table: the
    same bits as the dense tensors"""
    real, which, rows = step_inputs(cuda, bank, name)
    fn = step_fn(which, rows)
    want = fn(*real)
    other = []
    for key, t in zip(which, real):
        if key == "table":
            s = t.t().contiguous().t()
        elif t.dim() == 3:  # [N, P, d] points: frames behind an offset, the point rows padded
            wide = torch.full((t.shape[0] + 1, t.shape[1], t.shape[2] + 1), float("nan"), device=cuda)
            wide[1:, :, :t.shape[2]] = t
            s = wide[1:, :, :t.shape[2]]
        else:
            s = strided(t)
        assert torch.equal(s, t) and (key == "table" or s.storage_offset() > 0), key
        assert key == "table" or not s.is_contiguous() or s.shape[0] == 1, key  # (a single row is dense whatever its stride says)
        other.append(s)
    for key, a, b in zip(NAMES, fn(*other), want):
        assert torch.equal(bits(a), bits(b)), key


from tests.test_gpu_side_stream import delay  # noqa: E402,F401  (the session's calibrated delay, as that file measures it)


@case_ids
def test_side_stream_behind_a_delay(cuda, delay, bank, name):  # noqa: F811
    """the step on a side stream whose inputs arrive after the delay kernel: a launch on any other stream would read the stale
    buffers (NaN records and points, a table of zeros).  Both outputs have the default stream's bits."""
    from tests import test_gpu_side_stream as SS

    real, which, rows = step_inputs(cuda, bank, name)
    SS.run_family(delay, f"2-D ground truth, {name}", real, step_fn(which, rows), NAMES, [SS.EXACT] * len(NAMES))


@case_ids
def test_graph_replay(cuda, bank, name):
    """one capture of the step, replayed on changed records and points: the eager default-stream call's bits"""
    from tests.test_gpu_graph_replay import capture

    sets = [step_inputs(cuda, bank, name, seed=s) for s in (0, 1)]
    which, rows = sets[0][1:]
    assert sets[1][2] == rows
    fn = step_fn(which, rows)
    eager = [fn(*s[0]) for s in sets]
    torch.cuda.synchronize()
    assert not torch.equal(sets[0][0][0], sets[1][0][0])
    static = [t.clone() for t in sets[0][0]]
    graph, side, out = capture(lambda: fn(*static))
    torch.cuda.synchronize()
    graph.replay()  # (a capture runs nothing: the outputs exist from the first replay on)
    torch.cuda.synchronize()
    for key, a, b in zip(NAMES, out, eager[0]):
        assert torch.equal(bits(a), bits(b)), f"first replay: {key} differs from the eager call"
    for s, t in zip(static, sets[1][0]):
        s.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    for key, a, b in zip(NAMES, out, eager[1]):
        assert torch.equal(bits(a), bits(b)), f"replay: {key} differs from the eager call on the same inputs"
    assert not torch.equal(bits(out[1]), bits(eager[0][1])), "the replay ran on the refreshed inputs"


# ---- through the dataset ------------------------------------------------------------------------------------------------------------
ITEMS = (0, 3, 4)
QUERIES = ("frame", "camintr", "joints3d", "handverts3d", "objverts3d", "objfaces", "objcanverts", "side", "affinetrans", "joints2d", "joints2d_trans", "objverts2d",
           "objverts2d_trans", "handverts2d", "handverts2d_trans")


@pytest.fixture(scope="module")
def dataset_batches(cuda):
    """the same dataset with points2d="host" and "device" (hands and objects on the device in both), the same seeds, through
    ``seq_extend_collate`` and ``assemble_batch``: computed once, left unchanged"""
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.models import synthnet
    from handobjectconsist_amd.utils import collate

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None)
    out, states, ds, collated = {}, {}, None, {}
    for where in ("host", "device"):
        ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(272, 248), seed=1, sides=("right", "left"), obj_models=3, mano_layer=layer)
        hs = handobjset.HandObjSet(ds, inp_res=(64, 64), sample_nb=2, sides="right", color_fn=None, queries=QUERIES, obj_geometry="device", hand_geometry="device",
                                   points2d=where)
        random.seed(21)
        np.random.seed(21)
        torch.manual_seed(21)
        batch = collate.seq_extend_collate([hs[i] for i in ITEMS], collate.EXTEND_QUERIES)
        states[where] = (random.getstate(), np.random.get_state()[1].tolist(), torch.get_rng_state())
        collated[where] = batch
        out[where] = handobjset.assemble_batch(batch, cuda, (64, 64), mano_layer=layer, obj_bank=ds.obj_bank)
    assert states["host"][0] == states["device"][0] and states["host"][1] == states["device"][1] and torch.equal(states["host"][2], states["device"][2])
    return ds, layer, out, collated


def test_points2d_device_equals_host_through_the_dataset(cuda, dataset_batches):
    from handobjectconsist_amd.datasets import gt2d, manogt, objgt

    ds, layer, out, collated = dataset_batches
    assert all(not set(d) & set(gt2d.KEYS) and tuple(d["gt2d_info"].shape) == (3, gt2d.GT2D_INFO_FLOATS) and tuple(d["gt2d_joints"].shape) == (3, 21, 2)
               for d in collated["device"])
    models = list(zip(ds.obj_bank.verts, ds.obj_bank.faces))
    flips = 0
    worst = 0.0
    for pos, (fa, fb, cb) in enumerate(zip(out["host"], out["device"], collated["device"])):
        assert fa.keys() == fb.keys() and not {"gt2d_info", "gt2d_joints", "obj_info", "hand_info"} & set(fb) and set(gt2d.KEYS) | {"affinetrans"} <= set(fb)
        for key in fa:
            if torch.is_tensor(fa[key]):
                assert fb[key].is_cuda and fa[key].dtype == fb[key].dtype and fa[key].shape == fb[key].shape, key
            if key not in gt2d.KEYS:
                assert torch.equal(fa[key], fb[key]) if torch.is_tensor(fa[key]) else fa[key] == fb[key], key
        assert fb["objverts2d"].shape[1] == fb["objverts2d_trans"].shape[1] == fb["objverts3d"].shape[1], "objverts2d pads in step with objverts3d"
        assert fb["affinetrans"].dtype == torch.float32 and tuple(fb["affinetrans"].shape) == (3, 3, 3)
        info = gt2d.unpack_gt2d_info(cb["gt2d_info"].numpy())
        obj = objgt.unpack_obj_info(cb["obj_info"].numpy())
        hand = manogt.unpack_hand_info(cb["hand_info"].numpy())
        cam = gt2d.hand_cam_verts(layer, hand["fullpose"], hand["shape"], hand["trans"], hand["cam_rot"], device=cuda).cpu().numpy()
        case = dict(camintr=info["camintr"], flip=info["flip"], width=info["width"], affine=info["affine"], groups=[3], model=obj["model"], pose=obj["pose"],
                    points3d=cam, points2d=None)
        flips += int(info["flip"].sum())
        got = {k: fb[k].cpu().numpy() for k in gt2d.KEYS}
        ref = R.step(case, models)
        ref[0]["joints2d"] = (fa["joints2d"].cpu().numpy(), np.zeros(got["joints2d"].shape), True)  # (the host's joints: bit for bit)
        worst = max(worst, R.check_step(f"through the dataset, frame position {pos}", [got], ref, info["affine"], [3]))
        host = {k: fa[k].cpu().numpy() for k in gt2d.KEYS}
        # the host-assembled batch: objects under twice the bound (both sides carry rounding), joints' transformed pixels
        # neighbours at most (both are one float64 evaluation of the same expression on the same float32 pixels)
        assert (np.abs(host["objverts2d"].astype(np.float64) - got["objverts2d"]) <= 2 * ref[0]["objverts2d"][1]).all()
        assert R.within_one_ulp(got["joints2d_trans"], host["joints2d_trans"]).all()
        # the hand: the host evaluates MANO on the CPU.  tests/test_gpu_mano_full.py holds the two evaluations to
        # 1e-5 (1 + max |v|) per coordinate; that much on p, through the bound's own propagation
        for i in range(3):
            p = cam[i].astype(np.float64)
            _, q = R.base_ref(p, np.full(p.shape, 1e-5 * (1.0 + np.abs(p).max())), info["camintr"][i], info["flip"][i], info["width"][i])
            assert (np.abs(host["handverts2d"][i].astype(np.float64) - got["handverts2d"][i]) <= q).all()
    assert 0 < flips < 6, "the frames mix mirrored and unmirrored hands"
    print(f"GT2D through the dataset: largest base error / bound {worst:.3f}")


def test_metrics_end_to_end(cuda, dataset_batches):
    """predictions = the transformed ground truth + a known pixel offset, fed to ``joints2d_base`` and ``objverts2d_mepe`` from the
    device-assembled batch and from the host-assembled one: no sanity warning, the offset's length in base pixels (|d| over the
    crop's scale, frame by frame) comes back, and the two batches agree.  Tolerance: the batches' inputs differ by at most the
    base bound on both sides (objects; the joints are equal) and one ulp of the transformed pixels mapped back by the inverse
    affine; the metric kernel itself rounds in float32 on coordinates up to W and on |pred| / scale -- sixteen roundings are
    allowed for on each."""
    from handobjectconsist_amd.netscripts import evaluate

    from handobjectconsist_amd.datasets import gt2d, objgt

    ds, layer, out, collated = dataset_batches
    models = list(zip(ds.obj_bank.verts, ds.obj_bank.faces))
    base_bound = 0.0
    for cb in collated["device"]:
        info, obj = gt2d.unpack_gt2d_info(cb["gt2d_info"].numpy()), objgt.unpack_obj_info(cb["obj_info"].numpy())
        case = dict(camintr=info["camintr"], flip=info["flip"], width=info["width"], groups=[3], model=obj["model"], pose=obj["pose"])
        base_bound = max(base_bound, float(R.step(case, models)[0]["objverts2d"][1].max()))
    offset = torch.tensor([3.0, -4.0], device=cuda)
    reported = {}
    for where in ("host", "device"):
        tm = evaluate.TrainMetrics(center_idx=9)
        results = [{"joints2d": d["joints2d_trans"] + offset, "obj_verts2d": d["objverts2d_trans"] + offset} for d in out[where]]
        tm.feed({"supervision": "data", "data": out[where]}, {}, results)
        torch.cuda.synchronize()
        assert tm.warnings() == [], tm.warnings()
        saved = tm.save_dict()
        reported[where] = (saved["joints2d_base_epe_mean"]["train"], saved["objverts2d_mepe"]["train"])
        print(f"GT2D metrics, {where}-assembled: joints2d_base {reported[where][0]:.6f} px, objverts2d_mepe {reported[where][1]:.6f} px")
    aff = torch.cat([d["affinetrans"] for d in out["device"]]).cpu().numpy().astype(np.float64)
    scale = np.sqrt(aff[:, 0, 0] ** 2 + aff[:, 1, 0] ** 2)
    expected = float(np.mean(5.0 / scale))
    biggest = max(float(d[k].abs().max()) for d in out["device"] for k in ("joints2d_trans", "objverts2d_trans", "joints2d", "objverts2d"))
    tol = (2 * 2 ** 0.5 * base_bound + 2 ** 0.5 * np.spacing(np.float32(biggest)) / scale.min()) + 16 * R.U * (272 + biggest / scale.min())
    for k in (0, 1):
        assert abs(reported["device"][k] - reported["host"][k]) <= tol, (reported, tol)
        assert abs(reported["device"][k] - expected) <= tol + 16 * R.U * expected, (reported, expected, tol)
