"""The training metrics without a device: the restated evaluator (tests/evalutil_ref.py) against hand-computed logs, the
threshold rounding argument, the cases and bounds of tests/eval_metric_cases.py (an fp32 numpy emulation of the kernel's
operation order stays inside the bound for every case; no expected distance of the layer test lies within its bound of a
threshold, so that its PCK comparison is exact), the MrEvalJob layout, the entry points' refusals (decided before any
launch), and the Python layer's dictionaries against the restatement."""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_metric_cases as C
from tests import evalutil_ref as R


# ---- the restated evaluator ---------------------------------------------------------------------------------------------------
def test_reference_one_row():
    ev = R.EvalUtil(num_kp=2)
    ev.feed(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), np.array([[3.0, 4.0, 0.0], [1.0, 1.0, 3.0]]))  # distances 5 and 2
    mean, per_joint, median, auc, curve, t = ev.get_measures(0, 10, 11)  # thresholds 0, 1, .. 10
    assert per_joint == [5.0, 2.0] and mean == 3.5 and median == 3.5
    # keypoint 0 counts from t = 5 on (6 of 11 thresholds), keypoint 1 from t = 2 on
    want0, want1 = (t >= 5).astype(float), (t >= 2).astype(float)
    assert np.array_equal(curve, 0.5 * (want0 + want1))
    # trapezoids of width 1 over [0, 10]: a step at 5 has area 5.5 (half a trapezoid on the rising edge), at 2 area 8.5
    assert auc == pytest.approx(0.5 * (5.5 + 8.5) / 10.0, abs=1e-15)


def test_reference_two_rows_even_median_and_a_distance_on_a_threshold():
    ev = R.EvalUtil(num_kp=1)
    ev.feed(np.array([[0.0, 0.0]]), np.array([[1.0, 0.0]]))   # 1.0: exactly on a threshold -> counts, because of <=
    ev.feed(np.array([[0.0, 0.0]]), np.array([[0.0, 4.0]]))   # 4.0
    mean, per_joint, median, auc, curve, t = ev.get_measures(0, 4, 5)
    assert mean == 2.5 and median == 2.5 and per_joint == [2.5]
    assert curve.tolist() == [0.0, 0.5, 0.5, 0.5, 1.0]
    assert auc == pytest.approx((0.25 + 0.5 + 0.5 + 0.75) / 4.0, abs=1e-15)


def test_reference_all_zero_distances_and_the_trapezoid_normalisation():
    ev = R.EvalUtil(num_kp=3)
    for _ in range(4):
        ev.feed(np.ones((3, 3)), np.ones((3, 3)))
    for lo, hi, steps in ((0, 0.2, 20), (0, 100, 100), (0.5, 3.0, 7)):
        mean, per_joint, median, auc, curve, t = ev.get_measures(lo, hi, steps)
        assert mean == 0 and median == 0 and per_joint == [0, 0, 0]
        assert np.array_equal(curve, np.ones(steps))
        assert auc == pytest.approx(1.0, abs=1e-14)  # a curve of ones has area hi - lo: the normalisation
        assert np.array_equal(t, np.linspace(lo, hi, steps))


def test_reference_empty_evaluator_is_nan():
    mean, per_joint, median, auc, curve, t = R.EvalUtil().get_measures(0, 0.2, 20)
    assert mean != mean and median != median and auc != auc and per_joint == [] and np.isnan(curve).all() and len(t) == 20
    # ... and a keypoint that was never fed (8 corners in a 21-keypoint evaluator) is skipped, not averaged as NaN
    ev = R.EvalUtil()
    ev.feed(np.zeros((8, 2)), np.ones((8, 2)))
    mean, per_joint, *_ = ev.get_measures(0, 100, 100)
    assert len(per_joint) == 8 and mean == pytest.approx(np.sqrt(2.0))


@pytest.mark.parametrize("rng", C.MEASURE_RANGES + [(0.1, 7.3, 50)], ids=str)
def test_rounded_down_thresholds_reproduce_the_mixed_comparison(rng):
    """numpy compares fp32 distances with the fp64 linspace values; the fp32 comparison against each threshold rounded toward
    -inf gives the same answer for every fp32 value -- shown on the fp32 neighbours of each threshold, where it could differ"""
    from handobjectconsist_amd.netscripts import evaluate

    t64, t32 = C.thresholds32(*rng)
    assert np.array_equal(t32, evaluate._nearest_below(t64)) and t32.dtype == np.float32
    assert (t32.astype(np.float64) <= t64).all() and (np.nextafter(t32, np.float32(np.inf)).astype(np.float64) > t64).all()
    assert (np.diff(t32) >= 0).all()
    for steps in range(-3, 4):
        d = t32.copy()
        for _ in range(abs(steps)):
            d = np.nextafter(d, np.float32(np.inf if steps > 0 else -np.inf))
        assert d.dtype == np.float32
        assert np.array_equal(d.astype(np.float64) <= t64, d <= t32), steps


# ---- cases and bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.feed_cases() + [C.nan_case()] + [C.layer_case(i) for i in range(len(C.LAYER_BATCHES))], ids=repr)
def test_fp32_emulation_stays_inside_the_bound(case):
    emulated = C.forward(case, np.float32)["out"]
    assert emulated.dtype == np.float32
    ratio = C.check(f"emulation {case}", emulated, case)
    assert ratio <= 1.0


def test_the_special_cases_are_what_they_claim():
    near, sing = C.near_singular_case(), C.singular_case()
    f = C.forward(near, np.float64)
    assert 100 < f["D"][1] / abs(f["det"][1]) < 1e5 and np.isfinite(C.reference(near)[1]).all()
    assert C.forward(sing, np.float64)["det"][1] == 0 and C.forward(sing, np.float32)["det"][1] == 0
    # a dataset affine is far from singular: its bound stays below a hundredth of a pixel (coordinates of up to ~2000
    # pixels after a scale of 0.3 is undone: an fp32 ulp there is 1.2e-4)
    ordinary = C.by_name("B2-K21-2d-affine")
    assert C.reference(ordinary)[1].max() < 1e-2
    assert all(C.by_name(n).pred.shape[0] == 2 for n in C.EIGHT_JOBS) and len(C.EIGHT_JOBS) == 8


def test_no_layer_distance_lies_within_its_bound_of_a_threshold():
    """the condition under which the layer test's PCK curve equals the restated evaluator's exactly"""
    t64, _ = C.thresholds32(*C.LAYER_RANGE)
    closest = np.inf
    for i in range(len(C.LAYER_BATCHES)):
        dist, bound = C.reference(C.layer_case(i))
        gap = np.abs(dist[..., None] - t64) - bound[..., None]
        assert (gap > 0).all(), f"feed {i}: a distance within its bound of a threshold"
        closest = min(closest, float(gap.min()))
    assert sum(C.LAYER_BATCHES) > 2 * C.LAYER_CAPACITY  # two growths: 8 -> 16 -> 32
    print(f"EVAL-METRICS layer feeds: the closest distance stays {closest:.3e} clear of every threshold")


# ---- the library, no device ------------------------------------------------------------------------------------------------------
def test_job_struct_layout_matches_the_binding():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.netscripts import evaluate

    out = (ctypes.c_int * 32)()
    n = _lib.load().mr_eval_job_layout(out, 32)
    fields = [f for f, _ in evaluate.MrEvalJob._fields_]
    assert n == 1 + len(fields)
    assert out[0] == ctypes.sizeof(evaluate.MrEvalJob)
    assert list(out[1:n]) == [getattr(evaluate.MrEvalJob, f).offset for f in fields]
    assert ctypes.sizeof(evaluate.MrEvalJob) * _lib.EVAL_MAX_JOBS <= 1024  # (the jobs travel in the kernel's argument block)
    assert _lib.load().mr_eval_job_layout(None, 4) == -1


def _job(**over):
    from handobjectconsist_amd.netscripts import evaluate

    j = dict(pred=0x1000, target=0x2000, affine=None, out=0x3000, num_points=21, dims=3, center=-1, mode=0, affine_target=0)
    j.update(over)
    job = evaluate.MrEvalJob()
    for k, v in j.items():
        setattr(job, k, v)
    return job


def test_refusals_are_decided_before_any_launch():
    """never-dereferenced pointers: every row returns before the first HIP call"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.netscripts import evaluate

    lib = _lib.load()
    feed = lambda jobs, B=2: lib.mr_eval_feed((evaluate.MrEvalJob * len(jobs))(*jobs), len(jobs), B, None)
    assert feed([_job()], B=0) == 0 and lib.mr_eval_feed(None, 0, 2, None) == 0
    assert lib.mr_eval_feed(None, 1, 2, None) == -1 and feed([_job()], B=-1) == -1
    assert feed([_job()] * 9) == -1
    for bad in (dict(pred=None), dict(target=None), dict(out=None), dict(pred=0x1002), dict(out=0x3001), dict(affine=0x4001, dims=2),
                dict(dims=1), dict(dims=4), dict(center=21), dict(center=-2), dict(affine=0x4000, dims=3), dict(num_points=0),
                dict(num_points=4097), dict(mode=3), dict(mode=-1)):
        assert feed([_job(**bad)]) == -1, bad
        assert feed([_job(), _job(**bad)]) == -1, bad  # (any job refuses the whole feed)
    ws = lib.mr_eval_measures_workspace_floats
    assert ws(1000, 21, 20) == 21000 and ws(0, 21, 20) == 0
    assert ws(-1, 21, 20) == -1 and ws(10, 0, 20) == -1 and ws(10, 21, -1) == -1 and ws(1 << 30, 21, 20) == -1
    P = ctypes.c_void_p
    m = lambda rows=10, K=21, T=20, log=0x1000, thr=0x2000, sums=0x3000, pck=0x4000, mid=0x5000, nf=0x6000, work=0x7000: \
        lib.mr_eval_measures(P(log), rows, K, P(thr), T, P(sums), P(pck), P(mid), P(nf), P(work), None)
    assert m(rows=0) == 0 and m(rows=0, T=2000) == 0
    assert m(rows=-1) == -1 and m(K=0) == -1 and m(T=-1) == -1
    for name in ("log", "thr", "sums", "pck", "mid", "nf", "work"):
        assert m(**{name: None}) == -1, name
        assert m(**{name: 0x1002}) == -1, name
    assert m(sums=0x3004) == -1  # (fp64: 8 bytes)
    assert m(T=1025) == -2


# ---- the Python layer, no device ---------------------------------------------------------------------------------------------------
def _fed_reference_evaluators(seed, names):
    rng = np.random.default_rng(seed)
    evs = {name: R.EvalUtil() for name in R.DEFAULT_CONFIG}
    for name in names:
        K, dims, scale = (8, 2, 20.0) if name == "corners2d_base" else (21, 2, 20.0) if name.endswith("base") else (21, 3, 0.05)
        for _ in range(5):
            gt = rng.standard_normal((K, dims))
            evs[name].feed(gt, gt + rng.standard_normal((K, dims)) * scale)
    return evs


def test_parse_evaluators_dictionary():
    from handobjectconsist_amd.netscripts import evaluate

    assert evaluate.DEFAULT_CONFIG == R.DEFAULT_CONFIG
    evs = _fed_reference_evaluators(1, ["joints3d", "joints2d_base", "corners2d_base"])
    got, want = evaluate.parse_evaluators(evs), R.parse(evs)
    assert list(got) == list(want) == list(R.DEFAULT_CONFIG)
    for name in want:
        assert set(got[name]) == set(R.RESULT_KEYS)
        for key in R.RESULT_KEYS:
            np.testing.assert_array_equal(np.asarray(got[name][key]), np.asarray(want[name][key]), err_msg=f"{name} {key}")
    assert got["joints3d_cent"]["epe_mean"] != got["joints3d_cent"]["epe_mean"]  # never fed: NaN
    custom = evaluate.parse_evaluators({"joints3d": evs["joints3d"]}, config={"joints3d": [0, 1.0, 5]})
    assert len(custom["joints3d"]["thresholds"]) == 5


def test_train_metrics_save_dict_against_the_restated_loop():
    """keys, sub-keys and the NaN filter: TrainMetrics.save_dict over restated EvalUtil objects and number-fed meters against
    the restated epoch_pass tail over the same objects"""
    from handobjectconsist_amd.netscripts import evaluate

    tm = evaluate.TrainMetrics()
    tm.evaluators = _fed_reference_evaluators(2, ["joints3d", "joints3d_cent"])
    tm.consist_evaluators = _fed_reference_evaluators(3, ["joints3d", "corners2d_base"])
    ref_meters, ref_consist = R.AverageMeters(), R.AverageMeters()
    for step in range(3):
        for name, val in (("recov_joint3d", 0.5 + step), ("reg_loss", 2.0 * step)):
            tm.avg_meters.add_loss_value(name, val)
            ref_meters.add_loss_value(name, val)
        for name, val in (("warp_consist", 0.25 * step), ("reg_loss", 1.0 + step)):
            tm.consist_avg_meters.add_loss_value(name, val)
            ref_consist.add_loss_value(name, val)
    got = tm.save_dict("train")
    want = R.epoch_save_dict("train", ref_meters, ref_consist, tm.evaluators, tm.consist_evaluators)
    assert got == want
    assert set(got) == {"recov_joint3d", "reg_loss", "warp_consist", "joints3d_epe_mean", "joints3d_cent_epe_mean", "corners2d_base_epe_mean"}
    assert got["reg_loss"] == {"train": 2.0, "consist": 2.0} and set(got["joints3d_epe_mean"]) == {"train", "consist"}
    assert set(got["corners2d_base_epe_mean"]) == {"consist"} and "joints2d_base_epe_mean" not in got
    assert set(tm.evaluator_results()) == {"joints3d", "joints3d_cent"}
    assert evaluate.TrainMetrics().save_dict("val") == {}  # nothing fed: every evaluator NaN, every one filtered


def test_cpu_tensors_raise_type_error():
    from handobjectconsist_amd.netscripts import evaluate

    pts, aff = torch.zeros(2, 21, 2), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(TypeError):
        evaluate.recover_back(pts, aff)
    with pytest.raises(TypeError):
        evaluate.DeviceEvalUtil().feed_batch(pts, pts)
    with pytest.raises(TypeError):
        evaluate.feed_evaluators({n: evaluate.DeviceEvalUtil() for n in evaluate.EVALUATOR_NAMES}, {"joints3d": torch.zeros(2, 21, 3)},
                                 {"recov_joints3d": torch.zeros(2, 21, 3)})
    with pytest.raises(TypeError):
        evaluate.feed_avg_meters(evaluate.DeviceAverageMeters(), {"objverts3d": torch.zeros(2, 30, 3)}, {"recov_objverts3d": torch.zeros(2, 30, 3)})
    mean, per_joint, *_ = evaluate.DeviceEvalUtil().get_measures(0, 0.2, 20)  # an empty evaluator needs no device
    assert mean != mean and per_joint == []


def test_sample_keys_by_string_by_enum_and_by_the_reference_enum():
    from enum import Enum

    from handobjectconsist_amd.datasets import queries

    theirs = Enum("BaseQueries", [m.name for m in queries.BaseQueries])  # a same-named enum from another module
    for sample in ({"joints3d": 1}, {queries.BaseQueries.JOINTS3D: 1}, {theirs.JOINTS3D: 1}):
        assert queries.lookup(sample, "joints3d") == 1
    assert queries.PATH_KEYS["affinetrans"] is queries.TransQueries.AFFINETRANS
    assert queries.PATH_KEYS["objverts3d"] is queries.BaseQueries.OBJVERTS3D  # (an entry from before: unchanged)
