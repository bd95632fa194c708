"""Generate tests/golden/mano_bits.json: SHA-256 digests of what the MANO kernels (csrc/mano_lbs.hip) compute, values and
gradients, taken through ``SynthManoLayer.forward`` / ``forward_full`` on an MI355X.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mano_bits.py [output path]

tests/test_gpu_mano_grads.py holds the kernels to a yardstick against an fp64 oracle and the two entry points to each other;
a change that moved both entry points' bits together, inside the yardstick, would pass there.  This file is a record of the
kernels as they were while the pre / skin kernels and their adjoints were still templates on ``bool FULL``, one instantiation
per entry-point pair (the library's ``build.source_hash()`` at that commit is stored with it).  It is not regenerated from
later code: a digest that differs is a changed result.  tests/test_gpu_mano_bits.py imports the cases and the runner from
this file.

Cases, all from tests/geom_grad_cases.py: every variant of ``MANO_VARIANTS`` (both pose forms; centre none / 9 / tips 4, 8, 20;
translation absent / given / all zero; both entry points) x every run of ``MANO_RUNS`` (B = 1 twice, 32, 33: the blend
kernels' tile edges) x every pattern of ``MANO_WEIGHTS`` (unused outputs = NULL incoming gradients; all zero = the +0 rule of
grad trans).  Then the three epilogue cases of test_gpu_mano_full.py::test_forward_full_epilogue_on_verts_and_joints, values
only.  Per case: a digest of the raw bytes of every input (pose, betas, trans, the epilogue's arrays, and the layer's
constants as the kernels read them -- two of those are products made on the device) and of every output (verts, joints,
grad pose, grad betas, grad trans where there is a translation).

``main`` takes every digest twice and records a case only if both runs agree; it names the others.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, "mano_bits.json")

from oracle import mano_ref as M  # noqa: E402
from tests import geom_grad_cases as C  # noqa: E402

GRAD_CASES = [(v, r, w) for v in C.MANO_VARIANTS for r in C.MANO_RUNS for w in C.MANO_WEIGHTS]
# name -> (use_pca, center_idx, with_trans, post on the device): test_forward_full_epilogue_on_verts_and_joints
EPILOGUE_CASES = {"centre9-translated": (True, 9, True, True), "tip-centre": (True, 8, False, False),
                  "axisang-uncentred": (False, None, False, True)}
CASES = ["-".join(c) for c in GRAD_CASES] + ["epilogue-" + k for k in EPILOGUE_CASES]


def digest(t):
    a = t.detach().contiguous().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _consts_digest(layer):
    h = hashlib.sha256()
    for t in layer.hip_constants()["tensors"]:
        h.update(b"-" if t is None else t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _grad_layer(variant, dev):
    return C.make_layer(variant).to(dev)


def _grad_case(variant, run, pattern, dev):
    layer = _grad_layer(variant, dev)
    pose, betas, trans, wv, wj = C.mano_case_inputs(variant, run, pattern)
    out = C.mano_run(layer, C.MANO_VARIANTS[variant][0], pose, betas, trans, wv, wj)
    ins = {"pose": pose, "betas": betas, "consts": _consts_digest(layer)}
    ins.update({k: a for k, a in (("trans", trans), ("weights verts", wv), ("weights joints", wj)) if a is not None})
    names = {"verts": "verts", "joints": "joints", "pose": "grad pose", "betas": "grad betas", "trans": "grad trans"}
    return ins, {names[k]: v for k, v in out.items()}


def _epilogue_case(name, dev):
    from handobjectconsist_amd.models import synthnet

    use_pca, center_idx, with_trans, on_device = EPILOGUE_CASES[name]
    layer = synthnet.SynthManoLayer(ncomps=15, use_pca=use_pca, flat_hand_mean=not use_pca, center_idx=center_idx).to(dev)
    B, g, rng = 3, torch.Generator().manual_seed(17), np.random.default_rng(17)
    pose, betas = 0.4 * torch.randn(B, 18 if use_pca else 48, generator=g), torch.randn(B, 10, generator=g)
    trans = 0.1 * torch.randn(B, 3, generator=g) if with_trans else None
    rot = M.batch_rodrigues(rng.standard_normal((B, 3))).astype(np.float32)
    t1, t2 = (rng.standard_normal((B, 3)) * 0.3).astype(np.float32), (rng.standard_normal((B, 3)) * 0.3).astype(np.float32)
    post = {"scale": 1e-3, "trans": t1, "rot": rot, "trans2": t2}
    if on_device:
        post = {k: (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a) for k, a in post.items()}
    verts, joints = layer.forward_full(pose.to(dev), betas.to(dev), None if trans is None else trans.to(dev), post=post)
    ins = {"pose": pose, "betas": betas, "post rot": rot, "post trans": t1, "post trans2": t2, "consts": _consts_digest(layer)}
    if trans is not None:
        ins["trans"] = trans
    return ins, {"verts": verts, "joints": joints}


def digests(case, dev):
    """(inputs, outputs) of the case named ``case``: dicts name -> SHA-256 of the raw bytes"""
    if case.startswith("epilogue-"):
        ins, outs = _epilogue_case(case[len("epilogue-"):], dev)
    else:
        ins, outs = _grad_case(*GRAD_CASES[CASES.index(case)], dev)
    torch.cuda.synchronize(dev)
    as_digest = lambda d: {k: v if isinstance(v, str) else digest(v) for k, v in d.items()}
    return as_digest(ins), as_digest(outs)


def main():
    from handobjectconsist_amd import build

    dev = torch.device("cuda:0")
    res = {"source_hash": build.source_hash(), "device": torch.cuda.get_device_name(dev), "cases": {}}
    first = {case: digests(case, dev) for case in CASES}
    unstable = []
    for case in CASES:
        again = digests(case, dev)
        if again != first[case]:
            unstable.append(case)
            print(f"NOT RECORDED, two runs differ: {case}: "
                  f"{sorted(k for k in again[1] if again[1][k] != first[case][1].get(k))}")
            continue
        res["cases"][case] = {"inputs": again[0], "outputs": again[1]}
        print(case, " ".join(f"{k}={v[:8]}" for k, v in again[1].items()))
    out_path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{out_path}: {len(res['cases'])} of {len(CASES)} cases, {len(unstable)} unstable, "
          f"library source hash {res['source_hash'][:12]}")


if __name__ == "__main__":
    main()
