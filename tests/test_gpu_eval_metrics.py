"""mr_eval_feed / mr_eval_measures (csrc/eval_metrics.hip) and netscripts/evaluate.py on a device: the training metrics.

Feed: every distance element by element against the fp64 evaluation of the header's formulas under tests/eval_metric_cases.py's
bound (computed from the inputs; nothing is taken from a run), at (B, K) = (1, 1) .. (1, 4096) and per-sample sums of up to
10 000 points, with and without an affine, with every centre; eight jobs in one call against one per call; two calls; a
sample alone against the same sample in a batch; a singular affine and a NaN prediction poison their own rows only; the
refusals leave NaN-filled outputs untouched.  Measures: PCK counts, the two middle order statistics and the non-finite counts
exactly against numpy applied to the very log the device holds, the fp64 sums within rows x 2^-53 x sum |d|.  The layer:
DeviceEvalUtil against the restated EvalUtil (tests/evalutil_ref.py) over feeds that grow the log twice, the feeding rules on
enum-keyed, string-keyed and sparse samples, one launch and no host read per fed frame, epoch_pass with metrics against
without.  Guard bands, a side stream behind a delay and one hipGraph capture replayed twice (a capture pins the row offset the
feed writes at: a replay rewrites the same rows), in tests/test_gpu_mano_adapt.py's arrangement -- the host recorder does not
link this source.  Every output buffer is pre-filled with NaN (integers: a sentinel).

Measured on an MI355X (``EVAL-METRICS ...`` lines), largest error / bound: per-point distances 0.05 in 2-D without an affine,
0.06 with one (both at (1, 4096); 0.06 in the near-singular case, whose bound is 1 pixel), 0.24 in 3-D with a centre
((1, 4096), centre 9); per-sample sums 0.02 (K = 1; below 0.001 at K = 10 000, whose bound grows with K); recovered points 0.50
(3-D, centre 9: one subtraction against a 2 u bound).  In all 67 feed cases every output has the bits of the fp32 numpy emulation
of the operation order.  PCK counts, middle order statistics and non-finite counts equal numpy's in every log; the layer's mean
and median differ from the restated evaluator's by 7e-11 and 9e-11 (bound 2.2e-7); side stream: largest |side - default| 0 over
the eight jobs' outputs and the measures behind a 19.99 ms delay; guard bands: 24 allocations, 27 + 7 pointers inside them.  The
epoch test needs MIOpen's deterministic convolutions: with the default solvers two runs WITHOUT metrics differ in the last bits of
both losses.  The whole file takes 8 s, 5 of them the two epoch passes.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import eval_metric_cases as C
from tests import evalutil_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def stream_pool_left_where_it_was(cuda):
    """``torch.cuda.Stream()`` hands out the 32 streams of a pool in turn, and with four hardware queues one in four of them
    shares the default stream's queue (measured: a delayed copy on pool streams 6, 10, .. 30 is serialised with a default-stream
    read, on the others it is not).  tests/test_gpu_side_stream.py::test_the_mechanism_sees_a_stale_read, which runs after this
    file, needs a side stream that is not serialised, and which stream it gets depends on how many were made before it.  This
    file makes three (two side-stream families, one capture); with them that test got a serialised one.  So the file
    completes the round: afterwards the next stream of the pool is the one it was when the file started."""
    first = torch.cuda.Stream(cuda)
    yield
    made = 1
    while torch.cuda.Stream(cuda) != first:
        made += 1
        assert made <= 64, "the stream pool does not come round"
    for _ in range(31):
        torch.cuda.Stream(cuda)


def up(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def out_shape(case):
    B, K, dims = case.pred.shape
    return {C.PER_POINT: (B, K), C.PER_SAMPLE_SUM: (B,), C.POINTS: (B, K, dims)}[case.mode]


class Staged:
    """the device tensors of some cases and the MrEvalJob block over them"""

    def __init__(self, cuda, cases):
        from handobjectconsist_amd.netscripts import evaluate

        self.cases = list(cases)
        self.tensors = [(up(c.pred, cuda), up(c.target, cuda), up(c.affine, cuda)) for c in self.cases]
        self.outs = [torch.full(out_shape(c), float("nan"), dtype=torch.float32, device=cuda) for c in self.cases]
        self.block = (evaluate.MrEvalJob * len(self.cases))()
        for slot, c, (p, t, a), o in zip(self.block, self.cases, self.tensors, self.outs):
            slot.pred, slot.target, slot.affine, slot.out = p.data_ptr(), t.data_ptr(), (a.data_ptr() if a is not None else None), o.data_ptr()
            slot.num_points, slot.dims, slot.center, slot.mode, slot.affine_target = c.pred.shape[1], c.pred.shape[2], c.center, c.mode, \
                int(c.affine_target)

    def run(self, cuda, B=None):
        from handobjectconsist_amd import _lib

        _lib.call("mr_eval_feed", self.block, len(self.cases), self.cases[0].pred.shape[0] if B is None else B, _lib.stream_ptr(cuda))
        torch.cuda.synchronize()
        return self.outs


def run_case(cuda, case):
    return Staged(cuda, [case]).run(cuda)[0]


# ---- feed: values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.feed_cases(), ids=repr)
def test_feed_against_fp64(cuda, case):
    """every element under the bound; a second call has the same bits; how many elements differ from the fp32 emulation of the
    operation order is printed (none, where the division and the root round as IEEE's do)"""
    got = run_case(cuda, case)
    C.check(f"feed {case}", got.cpu().numpy(), case)
    again = run_case(cuda, case)
    assert torch.equal(bits(got), bits(again)), f"{case}: two calls differ"
    emulated = C.forward(case, np.float32)["out"]
    differ = int((emulated.view(np.uint32) != got.cpu().numpy().view(np.uint32)).sum())
    print(f"EVAL-METRICS feed {case}: {differ} of {emulated.size} elements differ from the fp32 emulation in bits")


def test_eight_jobs_in_one_call(cuda):
    cases = [C.by_name(n) for n in C.EIGHT_JOBS]
    together = Staged(cuda, cases).run(cuda)
    for case, got in zip(cases, together):
        C.check(f"eight jobs: {case}", got.cpu().numpy(), case)
        assert torch.equal(bits(got), bits(run_case(cuda, case))), f"{case}: in a call of eight it differs from the call alone"


@pytest.mark.parametrize("name", ["B3-K8-2d-affine", "B3-K8-3d-center7", "near-singular", "singular"])
def test_a_sample_does_not_depend_on_its_batch(cuda, name):
    case = C.by_name(name)
    batch, alone = run_case(cuda, case), run_case(cuda, case.rows(1, 2))
    assert torch.equal(bits(batch[1:2]), bits(alone)), f"{name}: sample 1 alone differs"
    first, rest = run_case(cuda, case.rows(0, 1)), run_case(cuda, case.rows(2, 3))
    assert torch.equal(bits(batch[0:1]), bits(first)) and torch.equal(bits(batch[2:3]), bits(rest))


def test_singular_affine_and_nan_prediction_poison_their_own_rows(cuda):
    for case in (C.singular_case(), C.nan_case()):
        got = run_case(cuda, case).cpu().numpy()
        C.check(f"poison {case}", got, case)  # (sample 1 non-finite, samples 0 and 2 under the bound)
        assert not np.isfinite(got[1]).any() and np.isfinite(got[[0, 2]]).all()
    # the same through a per-sample sum: one sum non-finite
    sing = C.singular_case()
    summed = C.Case("singular-sum", sing.pred.copy(), sing.target.copy(), sing.affine.copy(), mode=C.PER_SAMPLE_SUM, singular=(1,))
    C.check("poison singular-sum", run_case(cuda, summed).cpu().numpy(), summed)


def test_feed_refusals_launch_nothing(cuda):
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    case = C.by_name("B2-K21-2d-affine")
    for change, want in ((dict(dims=3), -1), (dict(center=21), -1), (dict(center=-2), -1), (dict(dims=4), -1), (dict(mode=5), -1),
                         (dict(num_points=4097), -1), (dict(pred=None), -1), (dict(out=1), -1)):
        st = Staged(cuda, [case, C.by_name("B2-K21-3d-center9")])
        for k, v in change.items():
            setattr(st.block[0], k, (st.outs[0].data_ptr() + v) if k == "out" else v)
        assert lib.mr_eval_feed(st.block, 2, 2, _lib.stream_ptr(cuda)) == want, change
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in st.outs), f"{change}: a refused feed wrote something"
    st = Staged(cuda, [case] * 8)
    nine = (type(st.block[0]) * 9)(*list(st.block), st.block[0])
    assert lib.mr_eval_feed(nine, 9, 2, _lib.stream_ptr(cuda)) == -1
    assert lib.mr_eval_feed(st.block, 8, 0, _lib.stream_ptr(cuda)) == 0 and lib.mr_eval_feed(st.block, 0, 2, _lib.stream_ptr(cuda)) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in st.outs)


# ---- measures ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xDEADBEEF


def run_measures(cuda, log, t32, stream_sync=True):
    """the raw entry point on NaN / sentinel-filled outputs -> (sums, counts, mid, nonfinite) as numpy arrays"""
    from handobjectconsist_amd import _lib

    rows, K = log.shape
    T = len(t32)
    dlog, dthr = up(log, cuda), up(t32, cuda)
    sums = torch.full((K,), float("nan"), dtype=torch.float64, device=cuda)
    counts = torch.full((K, T), SENTINEL - (1 << 32), dtype=torch.int32, device=cuda)
    mid = torch.full((K, 2), float("nan"), dtype=torch.float32, device=cuda)
    nonfinite = torch.full((K,), SENTINEL - (1 << 32), dtype=torch.int32, device=cuda)
    floats = _lib.load().mr_eval_measures_workspace_floats(rows, K, T)
    assert floats == rows * K
    work = torch.full((max(floats, 1),), float("nan"), dtype=torch.float32, device=cuda)
    P = _lib.ptr
    _lib.call("mr_eval_measures", P(dlog), rows, K, P(dthr), T, P(sums), P(counts), P(mid), P(nonfinite), P(work), _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert torch.equal(bits(dlog), bits(up(log, cuda))), "the log is read, not moved or changed"
    return sums.cpu().numpy(), counts.cpu().numpy().view(np.uint32), mid.cpu().numpy(), nonfinite.cpu().numpy().view(np.uint32)


def check_measures(what, log, rng, got):
    sums, counts, mid, nonfinite = got
    rows, K = log.shape
    t64, t32 = C.thresholds32(*rng)
    finite = np.isfinite(log)
    with np.errstate(invalid="ignore"):
        want_counts = np.stack([(log[:, k, None].astype(np.float64) <= t64[None, :]).sum(0) for k in range(K)])  # numpy's mixed comparison
    assert np.array_equal(counts, want_counts.astype(np.uint32)), f"{what}: PCK counts"
    assert np.array_equal(nonfinite, (~finite).sum(0).astype(np.uint32)), f"{what}: non-finite counts"
    srt = np.sort(log, axis=0)  # (NaN last)
    want_mid = np.stack([srt[(rows - 1) // 2], srt[rows // 2]], 1)
    assert np.array_equal(mid, want_mid, equal_nan=True), f"{what}: the middle order statistics"
    for k in range(K):
        col = log[:, k].astype(np.float64)
        if finite[:, k].all():
            exact = math.fsum(col.tolist())  # (the correctly rounded sum)
            bound = rows * 2.0 ** -53 * math.fsum(np.abs(col).tolist())
            assert abs(sums[k] - exact) <= bound, f"{what}: sums[{k}] {sums[k]} against {exact}"
        else:
            assert not np.isfinite(sums[k]) and (np.isnan(sums[k]) == bool(np.isnan(col).any())), f"{what}: sums[{k}]"


@pytest.mark.parametrize("rng", C.MEASURE_RANGES, ids=str)
def test_measures_against_numpy(cuda, rng):
    _, t32 = C.thresholds32(*rng)
    for name, log in C.measure_logs():
        check_measures(f"{name} {rng}", log, rng, run_measures(cuda, log, t32))


def test_measures_nonfinite_rows(cuda):
    """a NaN row and an inf row: counted in nonfinite, in no PCK bin; NaN sorts last, inf before it; the sum turns NaN / inf"""
    rng = (0, 0.2, 20)
    _, t32 = C.thresholds32(*rng)
    for rows in (3, 64, 1000):
        log = dict(C.measure_logs())[f"rows{rows}-K21"].copy()
        log[rows // 2, 4] = np.nan
        log[rows // 3, 5] = np.inf
        log[0, 6], log[rows - 1, 6] = np.nan, np.inf
        log[:, 7] = np.nan
        got = run_measures(cuda, log, t32)
        check_measures(f"non-finite rows{rows}", log, rng, got)
        assert got[3][4] == 1 and got[3][5] == 1 and got[3][6] == 2 and got[3][7] == rows
        assert got[1][4, -1] <= rows - 1 and got[1][5, -1] <= rows - 1 and got[1][6, -1] <= rows - 2 and got[1][7, -1] == 0
        assert np.isnan(got[0][4]) and np.isinf(got[0][5]) and np.isnan(got[2][7]).all()


def test_measures_two_calls_and_refusals(cuda):
    from handobjectconsist_amd import _lib

    _, t32 = C.thresholds32(0, 0.5, 20)
    log = dict(C.measure_logs())["rows4097-K21"]
    a, b = run_measures(cuda, log, t32), run_measures(cuda, log, t32)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "two calls differ"
    # rows == 0: MR_OK, outputs untouched; too many thresholds: refused, outputs untouched
    P = _lib.ptr
    outs = [torch.full((21,), float("nan"), dtype=torch.float64, device=cuda), torch.full((21, 1100), -7, dtype=torch.int32, device=cuda),
            torch.full((21, 2), float("nan"), device=cuda), torch.full((21,), -7, dtype=torch.int32, device=cuda)]
    dlog, thr, work = up(log, cuda), torch.zeros(1100, device=cuda), torch.full((log.size,), float("nan"), device=cuda)
    lib = _lib.load()
    assert lib.mr_eval_measures(P(dlog), 0, 21, P(thr), 20, *[P(o) for o in outs], P(work), _lib.stream_ptr(cuda)) == 0
    assert lib.mr_eval_measures(P(dlog), 4097, 21, P(thr), 1025, *[P(o) for o in outs], P(work), _lib.stream_ptr(cuda)) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs[0]).all()) and bool((outs[1] == -7).all()) and bool(torch.isnan(outs[2]).all()) and bool((outs[3] == -7).all())
    assert bool(torch.isnan(work).all())


# ---- the layer ----------------------------------------------------------------------------------------------------------------------
def test_device_eval_util_against_the_restated_evaluator(cuda):
    """uneven feeds that grow a log of capacity 8 twice; PCK curve and thresholds equal, mean / median / AUC within the
    distance bound carried through (tests/test_eval_metrics_host.py shows that no distance is within its bound of a threshold)"""
    from handobjectconsist_amd.netscripts import evaluate

    dev_eval, ref_eval = evaluate.DeviceEvalUtil(capacity=C.LAYER_CAPACITY), R.EvalUtil()
    bounds, capacities = [], []
    for i, (pred, target) in enumerate(C.layer_feeds()):
        dev_eval.feed_batch(up(pred, cuda), up(target, cuda))
        capacities.append(dev_eval.log.shape[0])
        for gt, pr in zip(target.astype(np.float64), pred.astype(np.float64)):
            ref_eval.feed(gt, pr)
        bounds.append(C.reference(C.layer_case(i))[1])
    assert capacities == [8, 16, 16, 32] and dev_eval.rows == sum(C.LAYER_BATCHES)
    bound = np.concatenate(bounds)  # [rows, 21]
    got, want = dev_eval.get_measures(*C.LAYER_RANGE), ref_eval.get_measures(*C.LAYER_RANGE)
    assert isinstance(got[0], float) and isinstance(got[2], float) and isinstance(got[3], float) and isinstance(got[1], list)
    assert np.array_equal(got[5], want[5]) and np.array_equal(got[4], want[4]), "thresholds and PCK curve"
    slack = 1e-12
    assert abs(got[0] - want[0]) <= bound.mean() + slack and abs(got[2] - want[2]) <= bound.max(0).mean() + slack
    assert np.all(np.abs(np.array(got[1]) - np.array(want[1])) <= bound.mean(0) + slack)
    assert abs(got[3] - want[3]) <= slack
    print(f"EVAL-METRICS layer: |mean - ref| {abs(got[0] - want[0]):.3e} (bound {bound.mean():.3e}), |median - ref| {abs(got[2] - want[2]):.3e}")
    # the log holds the raw entry point's bits, in feed order
    raw = torch.cat([run_case(cuda, C.layer_case(i)) for i in range(len(C.LAYER_BATCHES))])
    assert torch.equal(bits(dev_eval.log[:dev_eval.rows]), bits(raw))
    with pytest.raises(ValueError):
        dev_eval.feed_batch(torch.zeros(2, 8, 3, device=cuda), torch.zeros(2, 8, 3, device=cuda))
    # the per-sample call of the reference, and recover_back as a function
    one = evaluate.DeviceEvalUtil()
    one.feed(up(C.layer_feeds()[0][1][0], cuda), up(C.layer_feeds()[0][0][0], cuda))
    assert torch.equal(bits(one.log[:1]), bits(dev_eval.log[:1]))
    case = C.by_name("points-K21-affine")
    C.check("recover_back", evaluate.recover_back(up(case.pred, cuda), up(case.affine, cuda)).cpu().numpy(), case)


def _frame(cuda, seed, B=3, Vo=30):
    """(sample keyed by this package's enums, the same keyed by strings, results) with every quantity present"""
    from handobjectconsist_amd.datasets.queries import BaseQueries as BQ, TransQueries as TQ

    rng = np.random.default_rng(seed)
    aff = C.dataset_affines(rng, B).astype(np.float64)
    to_trans = lambda pts: (np.einsum("brc,bkc->bkr", aff, np.concatenate([pts, np.ones(pts.shape[:2] + (1,))], -1))[..., :2])
    j2, c2, v2 = (rng.uniform(0, 480, (B, K, 2)) for K in (21, 8, Vo))
    j3 = rng.uniform(-0.2, 0.2, (B, 21, 3)) + np.array([0.0, 0.0, 0.6])
    j3_trans = j3 @ np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # (the augmentation rotates the 3-D ground truth)
    v3 = rng.uniform(-0.1, 0.1, (B, Vo, 3)) + np.array([0.0, 0.0, 0.6])
    f32 = lambda a: up(a.astype(np.float32), cuda)
    enum_sample = {BQ.JOINTS2D: f32(j2), TQ.JOINTS2D: f32(to_trans(j2)), BQ.OBJCORNERS2D: f32(c2), TQ.OBJCORNERS2D: f32(to_trans(c2)),
                   BQ.OBJVERTS2D: f32(v2), TQ.OBJVERTS2D: f32(to_trans(v2)), TQ.AFFINETRANS: f32(aff), BQ.JOINTS3D: f32(j3),
                   TQ.JOINTS3D: f32(j3_trans), BQ.OBJVERTS3D: f32(v3)}
    names = {BQ.JOINTS2D: "joints2d", TQ.JOINTS2D: "joints2d_trans", BQ.OBJCORNERS2D: "objcorners2d", TQ.OBJCORNERS2D: "objcorners2d_trans",
             BQ.OBJVERTS2D: "objverts2d", TQ.OBJVERTS2D: "objverts2d_trans", TQ.AFFINETRANS: "affinetrans", BQ.JOINTS3D: "joints3d",
             TQ.JOINTS3D: "joints3d_trans", BQ.OBJVERTS3D: "objverts3d"}
    string_sample = {names[k]: v for k, v in enum_sample.items()}
    noise = lambda a, s: f32(a + rng.standard_normal(a.shape) * s)
    results = {"joints2d": noise(to_trans(j2), 5.0), "obj_corners2d": noise(to_trans(c2), 5.0), "obj_verts2d": noise(to_trans(v2), 5.0),
               "joints3d": noise(j3_trans, 0.02), "recov_joints3d": noise(j3, 0.02), "recov_objverts3d": noise(v3, 0.02),
               "obj_verts3d": noise(v3, 0.02)}
    return enum_sample, string_sample, results


def _host_frame_reference(sample, results, center=9):
    """the reference's feeding rules in fp64 numpy on host copies: {evaluator or meter: distances [B,K] or mean}"""
    s = {k: v.double().cpu().numpy() for k, v in sample.items()}
    r = {k: v.double().cpu().numpy() for k, v in results.items()}
    inv = np.linalg.inv(s["affinetrans"])
    back = lambda pts: np.einsum("brc,bkc->bkr", inv, np.concatenate([pts, np.ones(pts.shape[:2] + (1,))], -1))[..., :2]
    norm = lambda d: np.sqrt((d * d).sum(-1))
    cent = lambda a: a - a[:, center:center + 1]
    return {"joints2d_base": norm(back(r["joints2d"]) - s["joints2d"]), "corners2d_base": norm(back(r["obj_corners2d"]) - s["objcorners2d"]),
            "joints3d_cent": norm(cent(r["joints3d"]) - cent(s["joints3d_trans"])), "joints3d": norm(r["recov_joints3d"] - s["joints3d"]),
            "objverts2d_mepe": norm(back(r["obj_verts2d"]) - s["objverts2d"]).mean(),
            "objverts3d_mepe_trans": norm(r["recov_objverts3d"] - s["objverts3d"]).mean(),
            "sanity": norm(back(s["joints2d_trans"]) - s["joints2d"]).mean()}


def _new_sets():
    from handobjectconsist_amd.netscripts import evaluate

    return {n: evaluate.DeviceEvalUtil() for n in evaluate.EVALUATOR_NAMES}, evaluate.DeviceAverageMeters()


@pytest.mark.parametrize("keys", ["enums", "strings"])
def test_feeding_rules(cuda, monkeypatch, keys):
    """feed_evaluators and feed_avg_meters on a full frame: one launch each, the logs and meters against the reference's rules
    in fp64 on the host (pixels: 1e-2, a hundred fp32 ulps of a coordinate after the affine is undone; metres: 1e-6)"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.netscripts import evaluate

    enum_sample, string_sample, results = _frame(cuda, 11)
    sample = enum_sample if keys == "enums" else string_sample
    want = _host_frame_reference(string_sample, results)
    evaluators, meters = _new_sets()
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append(n), real_call(n, *a))[1])
    assert evaluate.feed_evaluators(evaluators, sample, results) == 1
    assert evaluate.feed_avg_meters(meters, sample, results) == 1
    monkeypatch.setattr(_lib, "call", real_call)
    assert calls == ["mr_eval_feed", "mr_eval_feed"]
    for name, tol in (("joints2d_base", 1e-2), ("corners2d_base", 1e-2), ("joints3d_cent", 1e-6), ("joints3d", 1e-6)):
        ev = evaluators[name]
        assert ev.rows == 3 and np.abs(ev.log[:3].double().cpu().numpy() - want[name]).max() <= tol, name
    assert evaluators["verts2d_base"].rows == 0
    assert abs(meters.average_meters["objverts2d_mepe"].avg - want["objverts2d_mepe"]) <= 1e-2
    assert abs(meters.average_meters["objverts3d_mepe_trans"].avg - want["objverts3d_mepe_trans"]) <= 1e-6
    # the sanity figure: recovered ground truth is the original up to fp32 rounding -- far below a pixel, no warning
    sums, points = evaluators["joints2d_base"].sanity[0]
    assert points == 21 and abs(float(sums.sum()) / (3 * 21) - want["sanity"]) <= 1e-2 and want["sanity"] < 1e-2
    assert evaluate._sanity_warnings("x", evaluators["joints2d_base"]) == []


def test_feeding_rules_absent_keys_and_the_two_deviations(cuda):
    from handobjectconsist_amd.netscripts import evaluate

    _, sample, results = _frame(cuda, 12)
    # a synthetic sample: 3-D ground truth only, no affine, no transformed entries; SynthMeshRegNet's result keys
    synth_sample = {k: sample[k] for k in ("joints3d", "objverts3d")}
    synth_results = {k: results[k] for k in ("recov_joints3d", "joints2d", "recov_objverts3d", "obj_verts2d")}
    evaluators, meters = _new_sets()
    assert evaluate.feed_evaluators(evaluators, synth_sample, synth_results) == 1
    assert evaluate.feed_avg_meters(meters, synth_sample, synth_results) == 1
    assert [n for n, e in evaluators.items() if e.rows] == ["joints3d_cent", "joints3d"]
    # deviation 2: without "joints3d" in the results the centred evaluator takes recov_joints3d
    cent = lambda a: a - a[:, 9:10]
    want = (cent(synth_results["recov_joints3d"].double()) - cent(sample["joints3d"].double())).norm(dim=-1)
    assert float((evaluators["joints3d_cent"].log[:3].double() - want).abs().max()) <= 1e-6
    # deviation 1: objverts3d_mepe_trans is fed on "recov_objverts3d" alone ("obj_verts3d" is not among the results)
    assert list(meters.average_meters) == ["objverts3d_mepe_trans"]
    parsed = evaluate.parse_evaluators(evaluators)
    assert parsed["joints2d_base"]["epe_mean"] != parsed["joints2d_base"]["epe_mean"] and parsed["joints3d"]["epe_mean"] > 0
    # nothing to feed: no launch, every evaluator NaN
    evaluators, meters = _new_sets()
    assert evaluate.feed_evaluators(evaluators, {"image": sample["joints3d"]}, synth_results) == 0
    assert evaluate.feed_avg_meters(meters, {}, synth_results) == 0
    assert all(v["epe_mean"] != v["epe_mean"] for v in evaluate.parse_evaluators(evaluators).values())
    # a None result counts as absent, as in the reference
    assert evaluate.feed_avg_meters(meters, sample, dict(results, obj_verts2d=None, recov_objverts3d=None)) == 0
    # a bad affine is reported at read-out
    tm = evaluate.TrainMetrics()
    broken = dict(sample, affinetrans=sample["affinetrans"] * 1.5)
    tm.feed({"data": [broken], "supervision": "data"}, {}, [dict(synth_results, obj_verts2d=None)])
    assert len(tm.warnings()) == 1 and "joints2d_base" in tm.warnings()[0]


def test_train_metrics_feed_is_one_launch_and_no_host_read(cuda, monkeypatch):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.netscripts import evaluate

    _, sample, results = _frame(cuda, 13)
    results = {k: results[k] for k in ("recov_joints3d", "joints2d", "recov_objverts3d", "obj_verts2d")}  # 7 jobs
    _, sample2, results2 = _frame(cuda, 14)
    losses = {"recov_joint3d": torch.tensor(0.5, device=cuda), "mano_reg_loss": torch.tensor([1.0, 3.0], device=cuda), "absent": None}
    data = {"data": [sample], "supervision": "data"}
    consist = {"data": [sample, sample2], "supervision": "consist"}
    tm = evaluate.TrainMetrics()
    torch.cuda.synchronize()
    calls = []
    real_call = _lib.call

    def forbidden(*a, **kw):
        raise AssertionError("a host read during feed")

    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append(n), real_call(n, *a))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", forbidden)
    monkeypatch.setattr(torch.Tensor, "item", forbidden)
    monkeypatch.setattr(torch.Tensor, "cpu", forbidden)
    tm.feed(data, losses, [results])
    assert calls == ["mr_eval_feed"]
    tm.feed(consist, losses, [results, results2])
    assert calls == ["mr_eval_feed", "mr_eval_feed"]
    with pytest.raises(ValueError):
        tm.feed({"data": [sample], "supervision": "other"}, losses, [results])
    monkeypatch.undo()
    torch.cuda.synchronize()
    saved = tm.save_dict("train")
    assert saved["recov_joint3d"] == {"train": 0.5, "consist": 0.5} and saved["mano_reg_loss"] == {"train": 2.0, "consist": 2.0}
    assert "absent" not in saved
    for name in ("joints2d_base_epe_mean", "joints3d_cent_epe_mean", "joints3d_epe_mean", "objverts2d_mepe", "objverts3d_mepe_trans"):
        assert set(saved[name]) == {"train", "consist"} and saved[name]["train"] == saved[name]["consist"] > 0, name
    assert "verts2d_base_epe_mean" not in saved and "corners2d_base_epe_mean" not in saved and tm.warnings() == []
    # a frame that carries every quantity has nine jobs, one more than a launch takes: two launches, the same numbers
    _, full_sample, full_results = _frame(cuda, 13)
    full = evaluate.TrainMetrics()
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append(n), real_call(n, *a))[1])
    del calls[:]
    full.feed(data, losses, [full_results])
    monkeypatch.undo()
    assert calls == ["mr_eval_feed", "mr_eval_feed"]
    full_saved = full.save_dict("train")
    assert full_saved["joints2d_base_epe_mean"]["train"] == saved["joints2d_base_epe_mean"]["train"] and "corners2d_base_epe_mean" in full_saved
    assert tm.consist_evaluators["joints3d"].rows == 3  # the first frame only


def test_epoch_pass_with_metrics(cuda):
    """two steps of SyntheticConsistLoader at B = 2, 64 x 64: the losses with metrics equal those without bit for bit, and
    joints3d_epe_mean is the value recomputed on the host from the results (3-D evaluators only: the synthetic samples carry
    no affine)"""
    from handobjectconsist_amd.models import synthnet, warpreg
    from handobjectconsist_amd.netscripts import epochpassconsist as EP, evaluate

    def run(metrics, spy=None):
        torch.manual_seed(0)
        model = synthnet.SynthMeshRegNet().to(cuda).eval()
        premodel = warpreg.WarpRegNet((64, 64), model, lambda_consist=0.001, lambda_data=0.999, criterion="l1", gt_refs=True,
                                      use_backward=True, mano_faces=model.mano_layer.th_faces, pair_outputs="loss").to(cuda)
        if spy is not None:
            real = premodel.forward
            premodel.forward = lambda batch: (lambda out: (spy.append((batch, out[2])), out)[1])(real(batch))
        # (a rate of 0: the vertex gradients meet in fp32 atomics -- tests/test_gpu_side_stream.py lists them -- so after a
        # real update two runs of the same steps differ in their last bits with or without metrics; every forward is exact)
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.0)
        loader = EP.SyntheticConsistLoader(2, image_size=64, steps=2, seed=3, device=cuda)
        return EP.epoch_pass(loader, premodel, opt, metrics=metrics)

    # (MIOpen's default convolution solvers are not run-to-run deterministic: measured, two runs WITHOUT metrics differ in the
    # last bits of both losses; with its deterministic solvers four runs, with and without metrics, gave the same bits)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        plain = run(None)
        seen, tm = [], evaluate.TrainMetrics()
        fed = run(tm, seen)
    finally:
        torch.backends.cudnn.deterministic = was
    assert len(plain) == len(fed) == 2
    for a, b in zip(plain, fed):
        assert torch.equal(bits(a), bits(b)), "metrics changed a loss"
    dists = []
    for batch, results in seen:
        if batch["supervision"] == "data":
            for sample, res in zip(batch["data"], results):
                dists.append((res["recov_joints3d"].detach().double() - sample["joints3d"].double()).norm(dim=-1).cpu().numpy())
    dists = np.concatenate(dists)
    saved = tm.save_dict("train")
    assert tm.evaluators["joints3d"].rows == dists.shape[0] == 4
    assert abs(saved["joints3d_epe_mean"]["train"] - dists.mean()) <= 1e-5 * max(1.0, float(dists.max()))
    assert "joints3d_cent_epe_mean" in saved and "objverts3d_mepe_trans" in saved and "joints2d_base_epe_mean" not in saved
    assert "consist" not in saved["joints3d_epe_mean"]  # the consist batches' first frame is unannotated: nothing to feed


def test_strided_inputs_are_made_dense(cuda):
    from handobjectconsist_amd.netscripts import evaluate

    case = C.by_name("B2-K21-2d-affine")
    pred, target, aff = up(case.pred, cuda), up(case.target, cuda), up(case.affine, cuda)
    want = evaluate.DeviceEvalUtil()
    want.feed_batch(pred, target, affine=aff)
    wide = torch.full((2, 23, 4), float("nan"), device=cuda)
    wide[:, 1:22, 1:3] = pred
    got = evaluate.DeviceEvalUtil()
    got.feed_batch(wide[:, 1:22, 1:3], target.transpose(0, 1).contiguous().transpose(0, 1), affine=aff.transpose(1, 2).contiguous().transpose(1, 2))
    assert not wide[:, 1:22, 1:3].is_contiguous()
    assert torch.equal(bits(got.log[:2]), bits(want.log[:2]))
    C.check("strided", got.log[:2].cpu().numpy(), case)
    double = evaluate.DeviceEvalUtil()
    double.feed_batch(pred.double(), target.double(), affine=aff.double())  # (other dtypes are cast)
    assert torch.equal(bits(double.log[:2]), bits(want.log[:2]))


# ---- memory and streams ---------------------------------------------------------------------------------------------------------
def _layer_feed_all(pred2, target2, aff, pred3, target3, verts_p, verts_t):
    """eight jobs through the layer -> the tensors they wrote"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.netscripts import evaluate as E

    evs = [E.DeviceEvalUtil(capacity=2) for _ in range(4)]
    meters = E.DeviceAverageMeters()
    jobs = [evs[0].job(pred2, target2, affine=aff), evs[1].job(pred2, target2), evs[2].job(pred3, target3, center=9),
            evs[3].job(pred3, target3), E._sanity_job(evs[0], target2, aff, pred2), meters.mean_job("a", verts_p, verts_t),
            meters.mean_job("b", pred2, target2, affine=aff)]
    points = torch.empty((pred2.shape[0], pred2.shape[1], 2), dtype=torch.float32, device=pred2.device)
    jobs.append(E.Job(pred2, None, points, affine=aff, mode=_lib.EVAL_POINTS))
    assert E._finish(jobs) == 1
    return [e.log[:e.rows] for e in evs] + [evs[0].sanity[0][0], meters.average_meters["a"].values[0].reshape(1),
                                                meters.average_meters["b"].values[0].reshape(1), points], jobs


def _layer_inputs(cuda, seed=0):
    rng = np.random.default_rng(500 + seed)
    p2, t2 = C._points(rng, 2, 21, 2)
    p3, t3 = C._points(rng, 2, 21, 3)
    vp, vt = C._points(rng, 2, 1000, 3)
    return [up(a, cuda) for a in (p2, t2, C.dataset_affines(rng, 2), p3, t3, vp, vt)]


LAYER_NAMES = ["log 2d affine", "log 2d", "log 3d centred", "log 3d", "sanity sums", "meter a", "meter b", "points"]


def test_guard_bands(cuda, monkeypatch):
    """a feed of all eight jobs and a measures call with every tensor inside guard bands: no band changes, every pointer of
    the job block and of the measures call lies inside a guarded interior, the values are those of the plain run"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.netscripts import evaluate as E
    from tests import guarded_alloc as G

    real = _layer_inputs(cuda)
    plain, _ = _layer_feed_all(*real)
    log = dict(C.measure_logs())["rows65-K21"]
    plain_eval = E.DeviceEvalUtil()
    plain_eval.log, plain_eval.rows, plain_eval.num_kp = up(log, cuda), 65, 21
    plain_measures = plain_eval.get_measures(0, 0.2, 20)
    torch.cuda.synchronize()
    alloc = G.GuardedAllocator(cuda)
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append((n, a)), real_call(n, *a))[1])
    alloc.install(monkeypatch)
    try:
        got, jobs = _layer_feed_all(*[alloc.guard(t) for t in real])
        guarded_eval = E.DeviceEvalUtil()
        guarded_eval.log, guarded_eval.rows, guarded_eval.num_kp = alloc.guard(up(log, cuda)), 65, 21
        got_measures = guarded_eval.get_measures(0, 0.2, 20)
        damage = alloc.check()
    finally:
        alloc.uninstall()
        monkeypatch.setattr(_lib, "call", real_call)
    assert not damage, "\n".join(damage)
    assert [n for n, _ in calls] == ["mr_eval_feed", "mr_eval_measures"]
    # the measures call's pointers are plain arguments; the feed's are the fields of its job block
    strangers = alloc.pointer_report([c for c in calls if c[0] == "mr_eval_measures"])
    assert not strangers and alloc.pointers_seen == 7, strangers
    block, n_jobs = calls[0][1][0], calls[0][1][1]
    assert n_jobs == 8
    inside = lambda p: any(a <= p < b for a, b in alloc.regions())
    seen = 0
    for slot in list(block)[:n_jobs]:
        for field in ("pred", "target", "affine", "out"):
            p = getattr(slot, field)
            if p:
                seen += 1
                assert inside(int(p)), f"job pointer {field} outside guarded storage"
    assert seen == 8 * 2 + 7 + 4  # pred and out everywhere, seven targets, four affines
    print(f"EVAL-METRICS guard bands: {alloc.count()} guarded allocations, {seen} + {alloc.pointers_seen} pointers inside them")
    for name, a, b in zip(LAYER_NAMES, got, plain):
        assert torch.equal(bits(a), bits(b)), name
    for a, b in zip(got_measures, plain_measures):
        assert np.array_equal(np.asarray(a), np.asarray(b))


from tests.test_gpu_side_stream import delay  # noqa: E402,F401  (the session's calibrated delay, as that file measures it)


def test_side_stream_behind_a_delay(cuda, delay):  # noqa: F811
    """a feed of eight jobs and a get_measures on a side stream whose inputs arrive after the delay: the default stream's bits"""
    from handobjectconsist_amd.netscripts import evaluate as E
    from tests import test_gpu_side_stream as SS

    real = _layer_inputs(cuda)
    SS.run_family(delay, "eval feed, eight jobs", real, lambda *t: _layer_feed_all(*t)[0], LAYER_NAMES, [SS.EXACT] * 8)

    def measures(log):
        ev = E.DeviceEvalUtil()
        ev.log, ev.rows, ev.num_kp = log, log.shape[0], log.shape[1]
        mean, per_joint, median, auc, curve, _ = ev.get_measures(0, 0.2, 20)
        return [torch.tensor([mean, median, auc] + per_joint + list(curve), dtype=torch.float64)]

    log = dict(C.measure_logs())["rows1000-K21"]
    SS.run_family(delay, "eval measures", [up(log, cuda)], measures, ["measures"], [SS.EXACT])


def test_graph_replay(cuda):
    """one capture of a feed, replayed twice on refreshed inputs: the captured rows are rewritten with the eager call's bits each
    time.  A capture pins the row offset (the `out` pointers are kernel arguments): a replay never appends."""
    from tests.test_gpu_graph_replay import capture

    sets = [_layer_inputs(cuda, seed) for seed in (0, 1, 2)]
    eager = [_layer_feed_all(*s)[0] for s in sets]
    torch.cuda.synchronize()
    static = [t.clone() for t in sets[0]]
    keep = []  # (the evaluators of the warm-up and captured calls: their logs are what the graph writes into)

    def call():
        out, jobs = _layer_feed_all(*static)
        keep.append(jobs)
        return out

    graph, side, out = capture(call)
    torch.cuda.synchronize()
    for k in (1, 2):
        for t, r in zip(static, sets[k]):
            t.copy_(r)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(LAYER_NAMES, out, eager[k]):
            if name.startswith("meter"):
                continue  # (the meters' means are torch ops behind the feed: captured too, compared through the sums below)
            assert torch.equal(bits(a), bits(b)), f"replay {k}: {name} differs from the eager call on the same inputs"
        assert not torch.equal(bits(out[0]), bits(eager[0][0])), "the replay ran on the refreshed inputs"
        for idx in (5, 6):
            assert torch.equal(bits(out[idx]), bits(eager[k][idx])), f"replay {k}: {LAYER_NAMES[idx]}"
