"""Training metrics from device tensors -- counterpart of meshreg/netscripts/evaluate.py (:8-18, :33-129) and of the two
libyana classes it feeds, ``EvalUtil`` (Zimmermann and Brox's PCK / AUC / end-point-error evaluator) and ``AverageMeters``,
under the reference's names.  The reference un-does the augmentation affine, takes per-keypoint distances and appends them to
Python lists on the host, behind about six ``.cpu()`` / ``.item()`` pipeline drains per fed frame.  Here a fed frame is ONE
launch of ``mr_eval_feed`` (csrc/eval_metrics.hip) that writes the distances into device-resident logs, and nothing is read
on the host until ``get_measures`` / ``.avg`` / ``TrainMetrics.save_dict`` ask for numbers (``mr_eval_measures``: exact PCK
counts, exact medians, fp64 sums).  DESIGN 20.

Two deviations from the reference's key tests, forced by ``SynthMeshRegNet``'s result keys (which do not change):

* ``objverts3d_mepe_trans`` is fed when ``"recov_objverts3d"`` is in the results.  The reference tests for ``"obj_verts3d"`` and
  then reads ``recov_objverts3d``.
* When ``"joints3d"`` is absent from the results but ``"recov_joints3d"`` is present, the centred evaluator ``joints3d_cent``
  takes the latter: the centring removes the difference (a translation).

Samples are read by plain string, by this package's enums or by the reference's own enums (``queries.lookup``).  A sample
keyed by strings that has no ``"..._trans"`` entry (no augmentation happened) gives its un-augmented entry in its place.
A frame that carries every 2-D and 3-D quantity feeds nine jobs, one more than a launch takes: it is fed in two launches;
every frame with at most eight is one.  The sanity figure of the reference (``recover_back`` of the transformed ground truth
against the original, warned about above 1 pixel) is kept per feed on the device and reported by ``warnings()`` at read-out.
CPU tensors raise ``TypeError`` like the rest of the path; non-dense or non-fp32 inputs are made dense fp32 here.
"""
import ctypes

import numpy as np
import torch

from handobjectconsist_amd import _lib
from handobjectconsist_amd.datasets import queries

_P, _I = ctypes.c_void_p, ctypes.c_int


class MrEvalJob(ctypes.Structure):
    """MrEvalJob of include/meshraster_hip.h (checked against mr_eval_job_layout by tests/test_eval_metrics_host.py)"""
    _fields_ = [("pred", _P), ("target", _P), ("affine", _P), ("out", _P), ("num_points", _I), ("dims", _I), ("center", _I),
                ("mode", _I), ("affine_target", _I), ("reserved", _I)]


DEFAULT_CONFIG = {
    "joints2d_base": [0, 100, 100],
    "corners2d_base": [0, 100, 100],
    "verts2d_base": [0, 100, 100],
    "joints3d_cent": [0, 0.2, 20],
    "joints3d": [0, 0.5, 20],
}
EVALUATOR_NAMES = tuple(DEFAULT_CONFIG)


class Job:
    """One job of a feed: the tensors (kept alive until the launch is issued) and where its distances go."""

    def __init__(self, pred, target, out, affine=None, affine_target=False, center=-1, mode=_lib.EVAL_PER_POINT):
        _lib.check_cuda(pred, target, affine, out)
        self.pred, self.target, self.affine = _lib.contig(pred.detach()), _lib.contig(None if target is None else target.detach()), \
            _lib.contig(None if affine is None else affine.detach())
        if self.pred.dim() != 3 or self.pred.shape[2] not in (2, 3):
            raise ValueError(f"evaluate: points must be [B, K, 2 or 3], got {list(self.pred.shape)}")
        if self.target is not None and self.target.shape != self.pred.shape:
            raise ValueError(f"evaluate: prediction {list(self.pred.shape)} and target {list(self.target.shape)} differ in shape")
        if self.affine is not None and tuple(self.affine.shape) != (self.pred.shape[0], 3, 3):
            raise ValueError(f"evaluate: the affine must be [B, 3, 3], got {list(self.affine.shape)}")
        self.out, self.affine_target, self.center, self.mode = out, bool(affine_target), -1 if center is None else int(center), mode


def run_jobs(jobs):
    """Issue the jobs: one ``mr_eval_feed`` per MR_EVAL_MAX_JOBS of them (all of one batch size, on one device)."""
    jobs = [j for j in jobs if j is not None]
    if not jobs:
        return 0
    B, dev = jobs[0].pred.shape[0], jobs[0].pred.device
    launches = 0
    for first in range(0, len(jobs), _lib.EVAL_MAX_JOBS):
        part = jobs[first:first + _lib.EVAL_MAX_JOBS]
        block = (MrEvalJob * len(part))()
        for slot, j in zip(block, part):
            if j.pred.shape[0] != B or j.pred.device != dev:
                raise ValueError("evaluate: the jobs of one feed share one batch size and one device")
            slot.pred, slot.target, slot.affine, slot.out = j.pred.data_ptr(), (j.target.data_ptr() if j.target is not None else None), \
                (j.affine.data_ptr() if j.affine is not None else None), j.out.data_ptr()
            slot.num_points, slot.dims, slot.center, slot.mode, slot.affine_target = j.pred.shape[1], j.pred.shape[2], j.center, j.mode, \
                int(j.affine_target)
        _lib.call("mr_eval_feed", block, len(part), B, _lib.stream_ptr(dev))
        launches += 1
    return launches


def recover_back(joints_trans, affinetrans):
    """Given 2d point coordinates [B,K,2] and an affine transform [B,3,3], recovers the original pixel points (the locations
    before the data augmentation): ``inverse(A) . [x, y, 1]``, first two rows -- one job of one feed."""
    _lib.check_cuda(joints_trans, affinetrans)
    B, K = joints_trans.shape[:2]
    out = torch.empty((B, K, 2), dtype=torch.float32, device=joints_trans.device)
    run_jobs([Job(joints_trans, None, out, affine=affinetrans, mode=_lib.EVAL_POINTS)])
    return out


def _nearest_below(thresholds64):
    """fp32 thresholds t' with (d <= t') == (d <= t) for every fp32 d: float32(t) rounded toward -inf"""
    t32 = thresholds64.astype(np.float32)
    above = t32.astype(np.float64) > thresholds64
    t32[above] = np.nextafter(t32[above], np.float32(-np.inf))
    return t32


_trapz = getattr(np, "trapezoid", None) or np.trapz


class DeviceEvalUtil:
    """``EvalUtil`` with its per-keypoint lists held as one ``[capacity, K]`` fp32 device log.  K is fixed by the first feed."""

    def __init__(self, num_kp=None, capacity=1024):
        self.num_kp, self.capacity, self.rows, self.log = num_kp, int(capacity), 0, None
        self.sanity = []  # (per-sample sums [B] of the sanity figure's distances, points per sample) per feed
        self._thresholds = {}

    def _reserve(self, B, K, device):
        """rows [self.rows, self.rows + B) of the log, grown by doubling through a stream-ordered copy"""
        if self.num_kp is None:
            self.num_kp = K
        if K != self.num_kp:
            raise ValueError(f"DeviceEvalUtil: fed {K} keypoints, the evaluator holds {self.num_kp}")
        need = self.rows + B
        if self.log is None or need > self.log.shape[0]:
            cap = self.capacity if self.log is None else self.log.shape[0]
            while cap < need:
                cap *= 2
            grown = torch.empty((cap, K), dtype=torch.float32, device=device)
            if self.rows:
                grown[:self.rows].copy_(self.log[:self.rows])
            self.log = grown
        elif self.log.device != device:
            raise ValueError(f"DeviceEvalUtil: the log is on {self.log.device}, the feed on {device}")
        out = self.log[self.rows:need]
        self.rows = need
        return out

    def job(self, pred, target, affine=None, center=-1):
        """the job that appends |pred - target| per keypoint for a batch (nothing is launched: ``run_jobs``)"""
        _lib.check_cuda(pred, target, affine)
        job = Job(pred, target, None, affine=affine, center=center)
        B, K = job.pred.shape[:2]
        if K > _lib.EVAL_MAX_POINTS:
            raise ValueError(f"DeviceEvalUtil: at most {_lib.EVAL_MAX_POINTS} keypoints")
        if B == 0:
            return None
        job.out = self._reserve(B, K, job.pred.device)
        return job

    def feed_batch(self, pred, target, affine=None, center=-1):
        """append the distances of a batch [B,K,2 or 3]; ``affine`` [B,3,3]: the prediction goes through ``recover_back`` first;
        ``center``: a keypoint subtracted from both sides"""
        run_jobs([self.job(pred, target, affine=affine, center=center)])

    def feed(self, keypoint_gt, keypoint_pred):
        """the reference's per-sample call: [K, 2 or 3] each"""
        self.feed_batch(keypoint_pred[None], keypoint_gt[None])

    def get_measures(self, val_min, val_max, steps):
        """(mean_k mean, [mean per keypoint], mean_k median, mean_k auc, mean_k pck[k, :], thresholds) as Python floats and
        numpy arrays; NaN where nothing was fed.  The one place that waits for the device."""
        thresholds = np.linspace(val_min, val_max, steps)
        if self.rows == 0:
            nan = float("nan")
            return nan, [], nan, nan, nan, thresholds
        if val_max < val_min:
            raise ValueError("get_measures: the thresholds must not decrease")
        K, T, dev = self.num_kp, int(steps), self.log.device
        key = (float(val_min), float(val_max), T)
        if key not in self._thresholds:
            self._thresholds[key] = torch.from_numpy(_nearest_below(thresholds)).to(dev)
        # one buffer, one copy to the host: sums f64 [K] | pck u32 [K,T] | mid f32 [K,2] | nonfinite u32 [K]
        sizes = [8 * K, 4 * K * T, 8 * K, 4 * K]
        offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        buf = torch.empty((offs[-1],), dtype=torch.uint8, device=dev)
        floats = _lib.load().mr_eval_measures_workspace_floats(self.rows, K, T)
        if floats < 0:
            raise RuntimeError("mr_eval_measures_workspace_floats failed: bad argument")
        work = torch.empty((max(int(floats), 1),), dtype=torch.float32, device=dev)
        base = buf.data_ptr()
        _lib.call("mr_eval_measures", _lib.ptr(self.log), self.rows, K, _lib.ptr(self._thresholds[key]), T, _P(base + offs[0]),
                  _P(base + offs[1]), _P(base + offs[2]), _P(base + offs[3]), _lib.ptr(work), _lib.stream_ptr(dev))
        host = buf.cpu().numpy()
        sums = host[offs[0]:offs[1]].view(np.float64)
        counts = host[offs[1]:offs[2]].view(np.uint32).reshape(K, T)
        mid = host[offs[2]:offs[3]].view(np.float32).reshape(K, 2).astype(np.float64)
        means = sums / self.rows
        # (numpy's median: NaN as soon as the column holds one -- the fp64 sum is NaN exactly then, distances being >= 0)
        medians = np.where(np.isnan(sums), np.nan, 0.5 * (mid[:, 0] + mid[:, 1]))
        pck = counts.astype(np.float64) / self.rows
        norm = _trapz(np.ones_like(thresholds), thresholds)
        with np.errstate(invalid="ignore", divide="ignore"):
            auc = _trapz(pck, thresholds, axis=1) / norm
        return float(means.mean()), [float(m) for m in means], float(medians.mean()), float(auc.mean()), pck.mean(0), thresholds


class DeviceAverageMeter:
    """``AverageMeter`` over 0-d device tensors: ``avg`` is the reference's running average with n = 1 per call, computed on
    request (one host read)."""

    def __init__(self):
        self.values = []  # 0-d tensors (views into a step's stack) or Python floats

    def update(self, val, n=1):
        if n != 1:
            raise ValueError("DeviceAverageMeter: the reference updates its meters with n = 1")
        self.values.append(val)

    @property
    def count(self):
        return len(self.values)

    @property
    def sum(self):
        if not self.values:
            return 0.0
        host = [float(v) for v in self.values if not torch.is_tensor(v)]
        dev = [v.detach().reshape(()) for v in self.values if torch.is_tensor(v)]
        total = float(np.sum(np.asarray(host, np.float64))) if host else 0.0
        if dev:
            total += float(torch.stack(dev).double().sum())
        return total

    @property
    def avg(self):
        return self.sum / self.count if self.values else 0.0


class DeviceAverageMeters:
    def __init__(self):
        self.average_meters = {}
        self.sanity = []

    def add_loss_value(self, loss_name, loss_val, n=1):
        """``loss_val``: a 0-d device tensor (not read) or a number"""
        if loss_name not in self.average_meters:
            self.average_meters[loss_name] = DeviceAverageMeter()
        self.average_meters[loss_name].update(loss_val.detach() if torch.is_tensor(loss_val) else loss_val, n=n)

    def add_loss_values(self, losses):
        """the losses of a step as one dict {name: tensor | None}: their means, stored by ONE stack-and-copy"""
        named = [(k, v.detach()) for k, v in losses.items() if v is not None and torch.is_tensor(v)]
        for k, v in losses.items():
            if v is not None and not torch.is_tensor(v):
                self.add_loss_value(k, v)
        if not named:
            return
        stacked = torch.stack([v.reshape(()) if v.numel() == 1 else v.float().mean() for _, v in named])
        for i, (k, _) in enumerate(named):
            self.add_loss_value(k, stacked[i])

    def mean_job(self, name, pred, target, affine=None):
        """the job behind a per-feed mean over B x V distances (``objverts2d_mepe`` and friends): per-sample sums from the feed
        kernel, the mean of the B sums on the device"""
        job = Job(pred, target, None, affine=affine, mode=_lib.EVAL_PER_SAMPLE_SUM)
        B, V = job.pred.shape[:2]
        if B == 0:
            return None
        job.out = torch.empty((B,), dtype=torch.float32, device=job.pred.device)
        job.after = lambda: self.add_loss_value(name, job.out.sum() / float(B * V))
        return job


def _finish(jobs):
    launches = run_jobs(jobs)
    for j in jobs:
        if j is not None and getattr(j, "after", None) is not None:
            j.after()
    return launches


def _sanity_job(owner, gt_trans, affine, original):
    """recover_back(transformed ground truth) against the original: per-sample sums, looked at by ``warnings()``"""
    job = Job(original, gt_trans, None, affine=affine, affine_target=True, mode=_lib.EVAL_PER_SAMPLE_SUM)
    B, K = job.pred.shape[:2]
    if B == 0:
        return None
    job.out = torch.empty((B,), dtype=torch.float32, device=job.pred.device)
    owner.sanity.append((job.out, K))
    return job


def _get(sample, name):
    try:
        return queries.lookup(sample, name)
    except KeyError:
        return None


def _get_trans(sample, name):
    got = _get(sample, name + "_trans")
    if got is None and queries.PATH_KEYS[name] not in sample and name in sample:
        got = sample[name]  # (a string-keyed sample without augmentation)
    return got


def _present(results, name):
    return name in results and results[name] is not None


def avg_meter_jobs(avg_meters, sample, results):
    jobs = []
    if _present(results, "obj_verts2d") and _get(sample, "objverts2d") is not None:
        gt_trans, affine, original = _get_trans(sample, "objverts2d"), _get(sample, "affinetrans"), _get(sample, "objverts2d")
        if gt_trans is None or affine is None:
            raise KeyError("feed_avg_meters: a sample with OBJVERTS2D needs TransQueries.OBJVERTS2D and AFFINETRANS")
        jobs.append(_sanity_job(avg_meters, gt_trans, affine, original))
        jobs.append(avg_meters.mean_job("objverts2d_mepe", results["obj_verts2d"], original, affine=affine))
    if _present(results, "recov_objverts3d") and _get(sample, "objverts3d") is not None:
        jobs.append(avg_meters.mean_job("objverts3d_mepe_trans", results["recov_objverts3d"], _get(sample, "objverts3d")))
    return jobs


def evaluator_jobs(evaluators, sample, results, idxs=None, center_idx=9):
    jobs = []
    for res_key, name, evaluator in (("joints2d", "joints2d", "joints2d_base"), ("obj_corners2d", "objcorners2d", "corners2d_base")):
        if _present(results, res_key) and _get(sample, name) is not None:
            gt_trans, affine, original = _get_trans(sample, name), _get(sample, "affinetrans"), _get(sample, name)
            if gt_trans is None or affine is None:
                raise KeyError(f"feed_evaluators: a sample with {name} needs its transformed entry and AFFINETRANS")
            jobs.append(_sanity_job(evaluators[evaluator], gt_trans, affine, original))
            jobs.append(evaluators[evaluator].job(results[res_key], original, affine=affine))
    pred3d = results["joints3d"] if _present(results, "joints3d") else results.get("recov_joints3d")
    if pred3d is not None and _get(sample, "joints3d") is not None:
        if center_idx is not None:
            gt_trans = _get_trans(sample, "joints3d")
            if gt_trans is None:
                raise KeyError("feed_evaluators: a sample with JOINTS3D needs TransQueries.JOINTS3D")
            jobs.append(evaluators["joints3d_cent"].job(pred3d, gt_trans, center=center_idx))
        if _present(results, "recov_joints3d"):
            jobs.append(evaluators["joints3d"].job(results["recov_joints3d"], _get(sample, "joints3d")))
    return jobs


def feed_avg_meters(avg_meters, sample, results):
    """evaluate.py:33-51: one ``mr_eval_feed``"""
    return _finish(avg_meter_jobs(avg_meters, sample, results))


def feed_evaluators(evaluators, sample, results, idxs=None, center_idx=9):
    """evaluate.py:54-98: one ``mr_eval_feed`` (``idxs`` is accepted and unused, as in the reference)"""
    return _finish(evaluator_jobs(evaluators, sample, results, idxs=idxs, center_idx=center_idx))


def feed_frame(avg_meters, evaluators, sample, results, center_idx=9):
    """both of the above for one frame in ONE ``mr_eval_feed``"""
    return _finish(avg_meter_jobs(avg_meters, sample, results) + evaluator_jobs(evaluators, sample, results, center_idx=center_idx))


RESULT_KEYS = ("epe_mean", "epe_mean_joints", "epe_median", "auc", "pck_curve", "thresholds")


def parse_evaluators(evaluators, config=None):
    """{evaluator name: {"epe_mean", "epe_mean_joints", "epe_median", "auc", "thresholds", "pck_curve"}} over the ranges of
    ``config`` ({name: [start, end, steps]}; None: the reference's defaults) -- evaluate.py:101-129's dictionary"""
    config = DEFAULT_CONFIG if config is None else config
    out = {}
    for name, evaluator in evaluators.items():
        start, end, steps = config[name][:3]
        mean, per_joint, median, auc, curve, thresholds = evaluator.get_measures(start, end, steps)
        out[name] = dict(zip(RESULT_KEYS, (mean, per_joint, median, auc, curve, thresholds)))
    return out


def _sanity_warnings(tag, owner):
    out = []
    for feed, (sums, points) in enumerate(owner.sanity):
        err = float(sums.double().sum()) / (sums.numel() * points)
        if err > 1 or err != err:
            out.append(f"{tag} feed {feed}: back to orig error on gt {err} > 1 pixel")
    return out


class TrainMetrics:
    """The evaluators and meters of epochpassconsist.py:34-51 -- one set for the data batches, one for the first frame of the
    consist batches -- fed as :69-84 feeds them and read out as :91-118 does."""

    def __init__(self, center_idx=9):
        self.evaluators = {name: DeviceEvalUtil() for name in EVALUATOR_NAMES}
        self.consist_evaluators = {name: DeviceEvalUtil() for name in EVALUATOR_NAMES}
        self.avg_meters = DeviceAverageMeters()
        self.consist_avg_meters = DeviceAverageMeters()
        self.center_idx = center_idx

    def feed(self, batch, all_losses, results):
        if "data" in batch["supervision"]:
            self.avg_meters.add_loss_values(all_losses)
            for sample, res in zip(batch["data"], results):
                feed_frame(self.avg_meters, self.evaluators, sample, res, center_idx=self.center_idx)
        elif "consist" in batch["supervision"]:
            self.consist_avg_meters.add_loss_values(all_losses)
            # Only compute metrics for weakly supervised frames (e.g. the first in the sequence)
            feed_frame(self.consist_avg_meters, self.consist_evaluators, batch["data"][0], results[0], center_idx=self.center_idx)
        else:
            raise ValueError(f"Supervision {batch['supervision']} not in [data|consist]")

    def save_dict(self, prefix="train"):
        """{name: {prefix | "consist": value}}: every meter's average, then ``<evaluator>_epe_mean`` for the evaluators that
        were fed (a NaN mean is left out) -- epochpassconsist.py:91-118.  Reads the device."""
        out = {}
        for name, meter in self.avg_meters.average_meters.items():
            out[name] = {prefix: meter.avg}
        for name, meter in self.consist_avg_meters.average_meters.items():
            out.setdefault(name, {})["consist"] = meter.avg
        for name, res in parse_evaluators(self.evaluators).items():
            if res["epe_mean"] == res["epe_mean"]:
                out[f"{name}_epe_mean"] = {prefix: res["epe_mean"]}  # (a fresh entry, as the reference makes it)
        for name, res in parse_evaluators(self.consist_evaluators).items():
            if res["epe_mean"] == res["epe_mean"]:
                out.setdefault(f"{name}_epe_mean", {})["consist"] = res["epe_mean"]
        return out

    def evaluator_results(self):
        """the third value the reference's epoch_pass returns: the data evaluators' results without the NaN ones"""
        return {name: res for name, res in parse_evaluators(self.evaluators).items() if res["epe_mean"] == res["epe_mean"]}

    def warnings(self):
        """the feeds whose sanity figure (recover_back of the transformed ground truth against the original) exceeded 1
        pixel; reads the device"""
        out = []
        for tag, meters, evaluators in (("data", self.avg_meters, self.evaluators), ("consist", self.consist_avg_meters, self.consist_evaluators)):
            out += _sanity_warnings(f"{tag} objverts2d", meters)
            for name, ev in evaluators.items():
                out += _sanity_warnings(f"{tag} {name}", ev)
        return out
