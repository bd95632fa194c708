"""A plain-numpy restatement of the evaluators the reference's training loop feeds (a checker like tests/jpeg_ref.py, nothing
pytest collects): ``EvalUtil`` -- Zimmermann and Brox's PCK / AUC / end-point-error evaluator in the form
``libyana.evalutils.zimeval`` carries it, whose ``get_measures`` also returns the per-keypoint means -- and ``AverageMeters``
(``libyana.evalutils.avgmeter``).  libyana is on no machine this suite runs on: the restatement follows the published
form and is NOT pinned against a run of it.

    feed(gt[K,d], pred[K,d]):   dist[k] = sqrt(sum_d (gt - pred)^2), appended to keypoint k's list
    get_measures(lo, hi, steps), t = linspace(lo, hi, steps), per keypoint k with data:
        mean_k, median_k of its list;  pck[k, j] = mean(data_k <= t[j]);  auc_k = trapz(pck[k], t) / trapz(1, t)
    -> (mean_k mean, [mean per keypoint], mean_k median, mean_k auc, mean_k pck[k, :], t); NaN when nothing was fed
"""
import warnings

import numpy as np

trapz = getattr(np, "trapezoid", None) or np.trapz


class EvalUtil:
    def __init__(self, num_kp=21):
        self.num_kp = num_kp
        self.data = [[] for _ in range(num_kp)]

    def feed(self, keypoint_gt, keypoint_pred, keypoint_vis=None):
        keypoint_gt, keypoint_pred = np.squeeze(keypoint_gt), np.squeeze(keypoint_pred)
        if keypoint_gt.ndim == 1:  # (one keypoint: squeeze took its axis too)
            keypoint_gt, keypoint_pred = keypoint_gt[None], keypoint_pred[None]
        vis = np.ones(keypoint_gt.shape[0], bool) if keypoint_vis is None else np.squeeze(keypoint_vis).astype(bool)
        assert keypoint_gt.ndim == 2 and keypoint_gt.shape == keypoint_pred.shape and vis.ndim == 1
        dist = np.sqrt(np.sum(np.square(keypoint_gt - keypoint_pred), axis=1))
        for k in range(keypoint_gt.shape[0]):
            if vis[k]:
                self.data[k].append(dist[k])

    def _get_epe(self, kp_id):
        data = np.array(self.data[kp_id])
        if len(data) == 0:
            return None, None
        return np.mean(data), np.median(data)

    def _get_pck(self, kp_id, threshold):
        data = np.array(self.data[kp_id])
        if len(data) == 0:
            return None
        return np.mean((data <= threshold).astype("float"))

    def get_measures(self, val_min, val_max, steps):
        thresholds = np.array(np.linspace(val_min, val_max, steps))
        norm_factor = trapz(np.ones_like(thresholds), thresholds)
        means, medians, aucs, curves = [], [], [], []
        for kp_id in range(self.num_kp):
            mean, median = self._get_epe(kp_id)
            if mean is None:
                continue
            means.append(mean)
            medians.append(median)
            curve = np.array([self._get_pck(kp_id, t) for t in thresholds])
            curves.append(curve)
            aucs.append(trapz(curve, thresholds) / norm_factor)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the mean of nothing: NaN, which is what the loop filters on)
            with np.errstate(invalid="ignore"):
                return (np.mean(np.array(means)), means, np.mean(np.array(medians)), np.mean(np.array(aucs)),
                        np.mean(np.array(curves), 0), thresholds)


class AverageMeter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class AverageMeters:
    def __init__(self):
        self.average_meters = {}

    def add_loss_value(self, loss_name, loss_val, n=1):
        if loss_name not in self.average_meters:
            self.average_meters[loss_name] = AverageMeter()
        self.average_meters[loss_name].update(loss_val, n=n)


DEFAULT_CONFIG = {"joints2d_base": [0, 100, 100], "corners2d_base": [0, 100, 100], "verts2d_base": [0, 100, 100],
                  "joints3d_cent": [0, 0.2, 20], "joints3d": [0, 0.5, 20]}
RESULT_KEYS = ("epe_mean", "epe_mean_joints", "epe_median", "auc", "pck_curve", "thresholds")


def parse(evaluators, config=DEFAULT_CONFIG):
    """what the reference's parse_evaluators makes of a dict of evaluators: {name: {RESULT_KEYS...}}"""
    out = {}
    for name, ev in evaluators.items():
        mean, per_joint, median, auc, curve, thresholds = ev.get_measures(*config[name][:3])
        out[name] = dict(zip(RESULT_KEYS, (mean, per_joint, median, auc, curve, thresholds)))
    return out


def epoch_save_dict(prefix, avg_meters, consist_avg_meters, evaluators, consist_evaluators):
    """the dictionary the reference's epoch_pass returns first (epochpassconsist.py:91-118): every meter's average under the
    pass's prefix, the consist meters' under "consist", then ``<evaluator>_epe_mean`` for every evaluator whose mean is not
    NaN -- a data evaluator's entry starts a fresh sub-dictionary, a consist evaluator's joins an existing one"""
    out = {}
    for name, meter in avg_meters.average_meters.items():
        out[name] = {prefix: meter.avg}
    for name, meter in consist_avg_meters.average_meters.items():
        out.setdefault(name, {})["consist"] = meter.avg
    for name, res in parse(evaluators).items():
        if res["epe_mean"] == res["epe_mean"]:
            out[f"{name}_epe_mean"] = {prefix: res["epe_mean"]}
    for name, res in parse(consist_evaluators).items():
        if res["epe_mean"] == res["epe_mean"]:
            out.setdefault(f"{name}_epe_mean", {})["consist"] = res["epe_mean"]
    return out
