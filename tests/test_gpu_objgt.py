"""mr_obj_bank_build / mr_obj_gt_batch (csrc/obj_gt.hip) and the layers above them on a device: ground-truth object meshes
gathered from a resident model bank.

Values: box, centre and canonical vertices of the bank bit for bit numpy's float32 (tests/objgt_ref.canonical), at the vertex
counts that cross a lane, a wave, a workgroup and its strides; a step's ``objverts3d`` element by element against the float64
evaluation under tests/objgt_ref.py's bound (gamma_9 times the magnitudes of the terms: nothing is taken from a run), its
``objcanverts``, ``objfaces`` (int64), ``objcantrans`` and ``objcanscale`` bit for bit -- cyclic padding down to a single row
repeated, two padded lengths in one launch.  Output buffers are pre-filled with NaN / -1 and are larger than the step: a slot
nobody writes, or a write past the step's rows, fails.

Also: through ``HandObjSet(obj_geometry="device")`` and ``assemble_batch(obj_bank=...)`` against the host path on the same seeds,
alone and with the other device paths; one consistency step of the network on a device-assembled batch; guard bands; strided
records and bank tensors; a side stream behind a delay (tests/test_gpu_side_stream.py's arrangement); one graph capture
replayed on changed records (tests/test_gpu_graph_replay.py's recipe) -- each of the four on every case of the value tests
(``CASES``) --; the refusals, with the outputs untouched.

Measured on an MI355X (``OBJGT ...`` lines): largest objverts3d error / bound 0.28 over the step cases (0.17 to 0.28), 0.20 through
the dataset on both paths; the pair step's loss 0.190376326 on both batches, largest |flow| 1.9 pixels; side stream: largest
|side - default| 0 over all eight outputs behind a 19.96 ms delay."""
import random

import numpy as np
import pytest
import torch

from tests import objgt_ref as R

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def up(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)


@pytest.fixture(scope="module")
def models():
    return R.bank_models()


@pytest.fixture(scope="module")
def bank(models):
    from handobjectconsist_amd.datasets import objgt

    return objgt.ObjectBank(models)


def to_numpy(groups):
    return [{k: v.cpu().numpy() for k, v in g.items()} for g in groups]


# ---- the bank ------------------------------------------------------------------------------------------------------------------
def raw_bank_build(cuda, models):
    """mr_obj_bank_build as it is, on NaN-filled outputs"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import objgt

    host = objgt.ObjectBank(models)
    d = {"verts": up(np.concatenate(host.verts), cuda), "table": up(host.table(), cuda)}
    M, V = len(host), d["verts"].shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)
    d.update(box=nan(M, 6), centre=nan(M, 3), canverts=nan(V, 3))
    P = _lib.ptr
    _lib.call("mr_obj_bank_build", P(d["verts"]), P(d["table"]), M, V, P(d["box"]), P(d["centre"]), P(d["canverts"]), _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    return d


def check_bank(what, d, models):
    lo = 0
    for k, (v, _) in enumerate(models):
        box, centre, can = R.canonical(v)
        for name, got, want in (("box", d["box"][k], box), ("centre", d["centre"][k], centre), ("canverts", d["canverts"][lo:lo + len(v)], can)):
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), f"{what}: {name} of model {k} ({len(v)} vertices)"
        lo += len(v)


def test_bank_build_is_numpy_bit_for_bit(cuda, models, bank):
    """all seven models in one bank (V = 1, 2, 63, 64, 65, 257, 1031) and each alone; the layer's bank is the raw call's"""
    d = raw_bank_build(cuda, models)
    check_bank("one bank", d, models)
    for k, m in enumerate(models):
        check_bank(f"model {k} alone", raw_bank_build(cuda, [m]), [m])
    layer = bank.on(cuda)
    for name in ("box", "centre", "canverts"):
        assert torch.equal(bits(layer[name]), bits(d[name])), name
    assert layer["faces"].dtype == torch.int32 and layer["faces"].shape == (sum(R.BANK_F), 3) and bank.on(cuda) is layer
    for k in range(len(models)):
        assert np.array_equal(bank.canonical(k)[0], d["canverts"][layer["table"][k, 0]:layer["table"][k, 0] + R.BANK_V[k]].cpu().numpy())


def test_bank_is_rebuilt_when_a_host_array_is_replaced(cuda, models):
    from handobjectconsist_amd.datasets import objgt

    b = objgt.ObjectBank(models[:3])
    first = b.on(cuda)
    moved = (models[1][0] + np.float32(0.25)).astype(np.float32)
    b.verts[1] = moved
    second = b.on(cuda)
    assert second is not first
    check_bank("after the replacement", second, [models[0], (moved, models[1][1]), models[2]])


def test_bank_zeros_of_both_signs(cuda):
    """-0 is below +0 on the device as in the host code, whatever the order in memory"""
    from handobjectconsist_amd.datasets import objgt

    for order in ([0.0, -0.0], [-0.0, 0.0]):
        v = np.array([[z, 1.0, -1.0] for z in order] * 40, np.float32)
        host = objgt.ObjectBank([(v, [[0, 1, 0]])])
        d = raw_bank_build(cuda, [(v, [[0, 1, 0]])])
        assert np.array_equal(d["box"][0].cpu().numpy().view(np.int32), host.box(0).view(np.int32))
        assert np.array_equal(d["canverts"].cpu().numpy().view(np.int32), host.canonical(0)[0].view(np.int32))


# ---- the step --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e-3], ids=["metres", "millimetres"])
@pytest.mark.parametrize("center", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("rot", [True, False], ids=["rotated", "unrotated"])
@pytest.mark.parametrize("flip", [True, False], ids=["mirrored", "unmirrored"])
def test_step_against_fp64(cuda, models, bank, flip, rot, center, scale):
    """five frames in two dicts: the one-vertex / one-face model padded to 65 / 129 rows in one and 257 / 128 in the other"""
    from handobjectconsist_amd.datasets import objgt

    args = R.step_args(R.FIVE["model"], flip, rot, center, scale)
    got = objgt.obj_geometry_batch(bank, groups=R.FIVE["groups"], device=cuda, **args)
    assert all(v.is_cuda for g in got for v in g.values()) and got[0]["objfaces"].dtype == torch.int64
    assert [tuple(g["objverts3d"].shape) for g in got] == [(3, 65, 3), (2, 257, 3)]
    R.check_step(f"device flip{flip} rot{rot} center{center} scale{scale}", to_numpy(got), R.step(models, groups=R.FIVE["groups"], **args))
    again = objgt.obj_geometry_batch(bank, groups=R.FIVE["groups"], device=cuda, **args)
    for a, b in zip(got, again):
        for k in objgt.KEYS:
            assert torch.equal(bits(a[k]), bits(b[k])), f"two calls differ: {k}"


@pytest.mark.parametrize("frames", [0, 1, 5, 7])
def test_step_sizes(cuda, models, bank, frames):
    """no frame, one, five in one dict, every model of the bank once (mixed mirrors): against fp64 and against the host path"""
    from handobjectconsist_amd.datasets import objgt

    ids = {0: [], 1: [6], 5: [2, 3, 4, 1, 0], 7: list(range(7))}[frames]
    args = R.step_args(ids, None, True, True, 1.0, seed=frames)
    got = objgt.obj_geometry_batch(bank, device=cuda, **args)
    R.check_step(f"device N={frames}", to_numpy(got), R.step(models, groups=[frames], **args))
    host = objgt.obj_geometry_host(bank, **args)
    for key in ("objcanverts", "objfaces", "objcantrans", "objcanscale"):
        assert np.array_equal(got[0][key].cpu().numpy(), host[0][key]), key
    if frames:  # both sides carry rounding: twice the bound
        ref = R.step(models, groups=[frames], **args)[0]
        assert (np.abs(got[0]["objverts3d"].cpu().numpy().astype(np.float64) - host[0]["objverts3d"]) <= 2 * ref["bound"]).all()


def raw_step(cuda, dbank, records, vrows, frows, spare=300, vcap=None, fcap=None):
    """mr_obj_gt_batch as it is: outputs filled with NaN / -1 and ``spare`` rows longer than the step; ``vcap`` / ``fcap``: the
    capacities the entry point is told, where not the buffers' own"""
    from handobjectconsist_amd import _lib

    n = records.shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)
    out = dict(objverts3d=nan(vrows + spare, 3), objcanverts=nan(vrows + spare, 3),
               objfaces=torch.full((frows + spare, 3), -1, dtype=torch.int64, device=cuda), objcantrans=nan(n + 1, 3), objcanscale=nan(n + 1))
    P = _lib.ptr
    rc = _lib.load().mr_obj_gt_batch(P(dbank["verts"]), P(dbank["canverts"]), P(dbank["centre"]), P(dbank["faces"]), P(dbank["table"]),
                                     dbank["table"].shape[0], dbank["verts"].shape[0], dbank["faces"].shape[0], P(records), n, vrows, frows,
                                     P(out["objverts3d"]), P(out["objcanverts"]), vrows + spare if vcap is None else vcap, P(out["objfaces"]),
                                     frows + spare if fcap is None else fcap,
                                     P(out["objcantrans"]), P(out["objcanscale"]), _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    return rc, out


def test_every_slot_is_written_and_nothing_else(cuda, models, bank):
    from handobjectconsist_amd.datasets import objgt

    args = R.step_args(R.FIVE["model"], None, True, True, 1.0)
    records, shapes, vrows, frows = objgt.frame_records(bank, groups=R.FIVE["groups"], **args)
    rc, out = raw_step(cuda, bank.on(cuda), up(records, cuda), vrows, frows)
    assert rc == 0
    want = objgt.obj_geometry_batch(bank, groups=R.FIVE["groups"], device=cuda, **args)
    for key, rows in (("objverts3d", vrows), ("objcanverts", vrows), ("objfaces", frows), ("objcantrans", 5), ("objcanscale", 5)):
        body, tail = out[key][:rows], out[key][rows:]
        flat = torch.cat([g[key].reshape((-1,) + tuple(body.shape[1:])) for g in want])
        assert torch.equal(bits(body), bits(flat)), f"{key}: the raw call and the layer differ"
        assert bool((tail == -1).all() if key == "objfaces" else torch.isnan(tail).all()), f"{key}: written past the step's rows"
        assert bool((body >= 0).all() if key == "objfaces" else torch.isfinite(body).all()), f"{key}: a slot nobody wrote"
    # a record whose padded length is shorter than its offsets say leaves the gap untouched, and a wild model id is clamped
    broken = records.copy()
    ints = broken.view(np.int32)
    ints[1, 1], ints[1, 2], ints[4, 0], ints[3, 0] = 10, 7, 1 << 30, -5
    rc, gap = raw_step(cuda, bank.on(cuda), up(broken, cuda), vrows, frows)
    assert rc == 0
    v1, f1 = ints[1, 4], ints[1, 5]
    assert bool(torch.isnan(gap["objverts3d"][v1 + 10:v1 + 65]).all()) and bool((gap["objfaces"][f1 + 7:f1 + 129] == -1).all())
    assert torch.equal(bits(gap["objverts3d"][:v1 + 10]), bits(out["objverts3d"][:v1 + 10]))
    last = R.canonical(models[6][0])[1]  # (frame 4: the id clamped to the bank's last model; frame 3: to model 0)
    assert np.array_equal(gap["objcantrans"][4].cpu().numpy(), last) and np.array_equal(gap["objcantrans"][3].cpu().numpy(), R.canonical(models[0][0])[1])
    assert bool(torch.isfinite(gap["objverts3d"][ints[3, 4]:vrows]).all())


def test_refusals_launch_nothing(cuda, models, bank):
    """null pointers, negative counts and capacities too small: MR_ERR_BADARG, the outputs still NaN / -1"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import objgt

    args = R.step_args(R.FIVE["model"], None, True, True, 1.0)
    records, _, vrows, frows = objgt.frame_records(bank, groups=R.FIVE["groups"], **args)
    dbank, rec = bank.on(cuda), up(records, cuda)
    untouched = lambda out: all(bool((t == -1).all() if t.dtype == torch.int64 else torch.isnan(t).all()) for t in out.values())
    for what, kw in (("vertex capacity", dict(vcap=vrows - 1)), ("face capacity", dict(fcap=frows - 1)), ("negative capacity", dict(fcap=-1)),
                     ("negative rows", dict(vrows=-1)), ("negative face rows", dict(frows=-1))):
        rc, out = raw_step(cuda, dbank, rec, kw.pop("vrows", vrows), kw.pop("frows", frows), **kw)
        assert rc == -1 and untouched(out), what
    rc, out = raw_step(cuda, dbank, rec[:0], 0, 0)  # no frame: nothing to do, nothing written
    assert rc == 0 and untouched(out)
    rc, out = raw_step(cuda, dbank, rec[:0], vrows, frows)  # rows without frames
    assert rc == -1 and untouched(out)
    for missing in ("verts", "canverts", "centre", "faces", "table"):
        rc, out = raw_step(cuda, dict(dbank, **{missing: _Null(dbank[missing])}), rec, vrows, frows)
        assert rc == -1 and untouched(out), missing
    lib, P = _lib.load(), _lib.ptr
    nan = torch.full((sum(R.BANK_V), 3), float("nan"), device=cuda)
    for bad in (dict(M=-1), dict(V=-1), dict(verts=None), dict(table=None)):
        rc = lib.mr_obj_bank_build(P(bad.get("verts", dbank["verts"])), P(bad.get("table", dbank["table"])), bad.get("M", 7), bad.get("V", sum(R.BANK_V)),
                                   P(nan), P(nan), P(nan), _lib.stream_ptr(cuda))
        torch.cuda.synchronize()
        assert rc == -1 and bool(torch.isnan(nan).all()), bad
    with pytest.raises(ValueError, match="outside the bank"):
        objgt.obj_geometry_batch(bank, [7], np.zeros((1, 3, 4)), device=cuda)
    with pytest.raises(ValueError, match="records must be"):
        objgt.run_records(dbank, rec[:, :31], vrows, frows)
    with pytest.raises(TypeError):
        objgt.run_records(dbank, rec.cpu(), vrows, frows)


class _Null:
    """stands in for a bank tensor whose pointer is NULL: the shape of the real one, a data pointer of 0"""

    def __init__(self, like):
        self.shape = like.shape

    def data_ptr(self):
        return 0


# ---- through the dataset ------------------------------------------------------------------------------------------------------------
ITEMS = (0, 3, 4)


def dataset_batches(cuda, opt_ins, poses=None, seed=21):
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.models import synthnet
    from handobjectconsist_amd.utils import collate

    layer = synthnet.SynthManoLayer(use_pca=False, flat_hand_mean=True, center_idx=None) if opt_ins.get("hand_geometry") == "device" else None
    out, states, ds, rows = {}, {}, None, None
    for geometry in ("host", "device"):
        ds = synthpose.SynthPoseDataset(num_pairs=3, frame_size=(272, 248), seed=1, sides=("right", "left"), obj_models=3, mano_layer=layer,
                                        jpeg_quality=90 if opt_ins.get("decode") == "device" else None)
        if poses is not None:
            ds.obj_infos = [(m, poses(p)) for m, p in ds.obj_infos]
        hs = handobjset.HandObjSet(ds, inp_res=(64, 64), sample_nb=2, sides="right", obj_geometry=geometry, **opt_ins)
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        batch = collate.seq_extend_collate([hs[i] for i in ITEMS], ["objverts3d", "objfaces", "objcanverts"])
        states[geometry] = (random.getstate(), np.random.get_state()[1].tolist(), torch.get_rng_state())
        if geometry == "device":
            assert all(not set(d) & {"objverts3d", "objfaces", "objcanverts"} and tuple(d["obj_info"].shape) == (3, 28) for d in batch)
            rows = [d["obj_info"].numpy() for d in batch]
        out[geometry] = handobjset.assemble_batch(batch, cuda, (64, 64), mano_layer=layer, obj_bank=ds.obj_bank if geometry == "device" else None)
    assert states["host"][0] == states["device"][0] and states["host"][1] == states["device"][1]
    assert torch.equal(states["host"][2], states["device"][2])
    return ds, out, rows


@pytest.mark.parametrize("opt_ins", [dict(color_fn=None), dict(color_fn="device", decode="device", hand_geometry="device")],
                         ids=["geometry-alone", "with-decode-colour-and-hands"])
def test_obj_geometry_device_equals_host_through_the_dataset(cuda, opt_ins):
    """same seeds -> same draws, RNG streams at the same position; faces and canonical vertices equal, objverts3d within twice
    the bound of the host path's (both sides carry rounding), every other key identical"""
    from handobjectconsist_amd.datasets import objgt

    ds, out, rows = dataset_batches(cuda, opt_ins)
    models = list(zip(ds.obj_bank.verts, ds.obj_bank.faces))
    args = objgt.unpack_obj_info(np.concatenate(rows))
    # the placements as the dataset holds them, in float64: frame position 0 is the item, position 1 its companion idx ^ 1
    args["pose"] = np.stack([ds.get_obj_info(i ^ pos)[1] for pos in (0, 1) for i in ITEMS])
    assert np.array_equal(args["pose"].astype(np.float32), objgt.unpack_obj_info(np.concatenate(rows))["pose"])
    assert args.pop("keys") == objgt.KEYS  # (the default queries ask for every object key)
    ref = R.step(models, groups=[len(ITEMS)] * 2, **args)
    assert len({len(models[m][0]) for m in args["model"][:3]}) > 1 and args["flip"].any() and not args["flip"].all()
    for name in ("host", "device"):
        got = [{k: (d[k].long() if k == "objfaces" else d[k]).cpu().numpy() for k in objgt.KEYS} for d in out[name]]
        R.check_step(f"through the dataset, {name} path", got, ref)
    for fa, fb in zip(out["host"], out["device"]):
        assert fa.keys() == fb.keys() and "obj_info" not in fb
        assert fb["objfaces"].is_cuda and fb["objfaces"].dtype == torch.int64 and torch.equal(fa["objfaces"].long(), fb["objfaces"])
        for key in ("objcanverts", "objcantrans", "objcanscale"):
            assert fa[key].dtype == fb[key].dtype and torch.equal(bits(fa[key]), bits(fb[key])), key
        for key in set(fa) - set(objgt.KEYS) - ({"handverts3d"} if "hand_geometry" in opt_ins else set()):
            same = torch.equal(fa[key], fb[key]) if torch.is_tensor(fa[key]) else fa[key] == fb[key]
            assert same, key


@pytest.mark.parametrize("queries", [("objverts3d", "objfaces"), ("objcanverts",), ("objfaces",)], ids="+".join)
def test_partial_queries_give_the_host_paths_keys(cuda, queries):
    """the row remembers which object queries were asked for: the device-assembled batch has the host-assembled batch's keys"""
    from handobjectconsist_amd.datasets import handobjset, objgt

    q = ("frame", "camintr", "joints3d", "side") + queries
    _, out, _ = dataset_batches(cuda, dict(color_fn=None, queries=q))
    for fa, fb in zip(out["host"], out["device"]):
        assert fa.keys() == fb.keys() and set(fb) & set(objgt.KEYS) and not set(objgt.KEYS) <= set(fb)
        for key in set(fa) & set(objgt.KEYS) - {"objverts3d"}:
            assert torch.equal(fa[key].long() if key == "objfaces" else fa[key], fb[key]), key


def test_pair_step_on_a_device_assembled_batch(cuda):
    """one pair step (warpbranch.forward, pair_outputs="loss", through WarpRegNet.warp_forward) on the device-assembled batch
    and on the host-assembled one, frame 0's meshes being its own ground truth (leaves that take a gradient).  The placements
    are pure translations, for which both paths round alike (v + b once; the rotation blocked): the two objverts3d are equal
    to the bit, and so must be the flows, the loss and the gradients.  The int64 faces of the device path are taken as they
    are."""
    from handobjectconsist_amd.models.synthnet import SynthMeshRegNet
    from handobjectconsist_amd.models.warpreg import WarpRegNet
    from handobjectconsist_amd.warping import opticalflow

    shift = lambda p: np.concatenate([np.eye(3), p[:, 3:]], 1)
    _, out, _ = dataset_batches(cuda, dict(color_fn=None, block_rot=True, spacing=1, center_idx=9), poses=shift)
    model = SynthMeshRegNet().to(cuda).eval()
    pre = WarpRegNet((64, 64), model, criterion="l1", gt_refs=True, use_backward=True, mano_faces=model.mano_layer.th_faces,
                     pair_outputs="loss").to(cuda)
    results = {}
    for geometry in ("host", "device"):
        samples = out[geometry]
        if geometry == "host":
            samples = [dict(s, objfaces=s["objfaces"].long()) for s in samples]
        leaves = [s[k].detach().clone().requires_grad_(True) for s in samples for k in ("handverts3d", "objverts3d")]
        all_results = [{"recov_handverts3d": leaves[2 * k], "recov_objverts3d": leaves[2 * k + 1]} for k in range(len(samples))]
        loss, pair = pre.warp_forward(samples, all_results)
        loss.backward()
        flows = [f.clone() for f in opticalflow.dense_flows(pair["recons_flows"][0])]
        print(f"OBJGT pair step, {geometry}-assembled: loss {float(loss.detach()):.9g}, largest |flow| {max(float(f.abs().max()) for f in flows):.4g}")
        assert torch.isfinite(loss) and float(loss.detach()) > 0 and max(float(f.abs().max()) for f in flows) > 0
        results[geometry] = [loss.detach()] + flows + [leaves[0].grad, leaves[1].grad]
    for fa, fb in zip(out["host"], out["device"]):
        assert torch.equal(bits(fa["objverts3d"]), bits(fb["objverts3d"])), "pure translations round alike on both paths"
    assert len(results["host"]) == len(results["device"]) == 5
    for k, (a, b) in enumerate(zip(results["host"], results["device"])):
        assert a is not None and torch.equal(bits(a), bits(b)), ("loss", "flow 1->2", "flow 2->1", "hand gradient", "object gradient")[k]
    assert float(results["device"][4].abs().max()) > 0, "the object's vertices take a gradient"


# ---- memory and streams ------------------------------------------------------------------------------------------------------------
NAMES = ["box", "centre", "canverts", "objverts3d", "objcanverts", "objfaces", "objcantrans", "objcanscale"]


# every step-kernel and bank-build case of the value tests above, once more: the sixteen combinations on the five frames in two
# dicts, the step sizes, and each model alone in its bank (two frames of it)
CASES = {f"five-{'mirrored' if f else 'unmirrored'}-{'rotated' if r else 'unrotated'}-{'centred' if c else 'uncentred'}-{'mm' if sc < 1 else 'm'}":
         dict(model=R.FIVE["model"], groups=R.FIVE["groups"], flip=f, rot=r, center=c, scale=sc)
         for f in (True, False) for r in (True, False) for c in (True, False) for sc in (1.0, 1e-3)}
CASES.update({"five-mixed-mirrors": dict(model=R.FIVE["model"], groups=R.FIVE["groups"]), "one-frame": dict(model=[6], groups=[1]),
              "five-frames-one-dict": dict(model=[2, 3, 4, 1, 0], groups=[5]), "seven-frames": dict(model=list(range(7)), groups=[7])})
CASES.update({f"model-{k}-alone": dict(model=[0, 0], groups=[2], alone=k) for k in range(len(R.BANK_V))})
case_ids = pytest.mark.parametrize("case", sorted(CASES))


def case_models(models, case):
    alone = CASES[case].get("alone")
    return models if alone is None else [models[alone]]


def step_inputs(cuda, models, case, seed=0):
    from handobjectconsist_amd.datasets import objgt

    c = CASES[case]
    bank = objgt.ObjectBank(case_models(models, case))
    args = R.step_args(c["model"], c.get("flip"), c.get("rot", True), c.get("center", True), c.get("scale", 1.0), seed=seed)
    records, _, vrows, frows = objgt.frame_records(bank, groups=c["groups"], **args)
    real = [up(records, cuda), up(np.concatenate(bank.verts), cuda), up(np.concatenate(bank.faces), cuda), up(bank.table(), cuda)]
    return real, vrows, frows


def build_and_step(vrows, frows):
    """(records, verts, faces, table) -> the bank build and the step on the current stream: NAMES"""
    from handobjectconsist_amd.datasets import objgt

    def fn(records, verts, faces, table):
        d = objgt.finish_device_bank({"verts": verts, "faces": faces, "table": table})
        return [d["box"], d["centre"], d["canverts"]] + list(objgt.run_records(d, records, vrows, frows))
    return fn


@case_ids
def test_guard_bands(cuda, monkeypatch, models, case):
    """bank build and step with every tensor inside guard bands: no band changes, every pointer the entry points get lies in a
    guarded interior, and the values are those of the plain run"""
    from handobjectconsist_amd import _lib
    from tests import guarded_alloc as G

    real, vrows, frows = step_inputs(cuda, models, case)
    fn = build_and_step(vrows, frows)
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
    print(f"OBJGT guard bands {case}: {alloc.count()} guarded allocations, {alloc.pointers_seen} pointer arguments")
    assert not damage, "\n".join(damage)
    assert not strangers, strangers
    assert [n for n, _ in calls] == ["mr_obj_bank_build", "mr_obj_gt_batch"] and alloc.pointers_seen == 5 + 11
    for name, a, b in zip(NAMES, got, plain):
        assert alloc.holds(a), f"{name}: not in guarded storage"
        assert torch.equal(bits(a), bits(b)), name


@case_ids
def test_strided_records_and_bank_tensors_are_made_dense(cuda, models, case):
    """records as a column slice of a wider tensor, vertices behind a storage offset with padded rows, a transposed table: the
    same bits as the dense tensors"""
    real, vrows, frows = step_inputs(cuda, models, case)
    fn = build_and_step(vrows, frows)
    want = fn(*real)
    records, verts, faces, table = real
    wide = torch.full((records.shape[0] + 2, 40), float("nan"), device=cuda)
    wide[1:-1, 3:35] = records
    inner = torch.full((verts.shape[0] + 1, 4), float("nan"), device=cuda)
    inner[1:, :3] = verts
    table_t = table.t().contiguous().t()
    faces_off = torch.cat([faces.new_zeros((1, 3)), faces])[1:]
    strided = (wide[1:-1, 3:35], inner[1:, :3], faces_off, table_t)
    assert strided[0].storage_offset() == 43 and strided[1].storage_offset() == 4 and faces_off.storage_offset() == 3
    for t in (strided[0], strided[1], table_t):  # (a single row is dense whatever its stride says)
        assert t.shape[0] == 1 or not t.is_contiguous()
    for name, a, b in zip(NAMES, fn(*strided), want):
        assert torch.equal(bits(a), bits(b)), name


from tests.test_gpu_side_stream import delay  # noqa: E402,F401  (the session's calibrated delay, as that file measures it)


@case_ids
def test_side_stream_behind_a_delay(cuda, delay, models, case):  # noqa: F811
    """bank build + step on a side stream whose inputs arrive after the delay kernel: a launch on any other stream would read the
    stale buffers (NaN vertices and records, a table of zeros).  Every output has the default stream's bits."""
    from tests import test_gpu_side_stream as SS

    real, vrows, frows = step_inputs(cuda, models, case)
    side = SS.run_family(delay, f"object ground truth, {case}", real, build_and_step(vrows, frows), NAMES, [SS.EXACT] * len(NAMES))
    check_bank(f"side stream, {case}", dict(zip(NAMES[:3], side[:3])), case_models(models, case))


@case_ids
def test_graph_replay(cuda, models, case):
    """one capture of bank build + step, replayed on changed records: the eager default-stream call's bits"""
    from tests.test_gpu_graph_replay import capture

    sets = [step_inputs(cuda, models, case, seed=s) for s in (0, 1)]
    vrows, frows = sets[0][1:]
    fn = build_and_step(vrows, frows)
    eager = [fn(*s[0]) for s in sets]
    torch.cuda.synchronize()
    assert not torch.equal(sets[0][0][0], sets[1][0][0])
    static = [t.clone() for t in sets[0][0]]
    graph, side, out = capture(lambda: fn(*static))
    torch.cuda.synchronize()
    graph.replay()  # (a capture runs nothing: the outputs exist from the first replay on)
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, out, eager[0]):
        assert torch.equal(bits(a), bits(b)), f"first replay: {name} differs from the eager call"
    static[0].copy_(sets[1][0][0])
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, out, eager[1]):
        assert torch.equal(bits(a), bits(b)), f"replay: {name} differs from the eager call on the same records"
    assert not torch.equal(bits(out[3]), bits(eager[0][3])), "the replay ran on the refreshed records"
