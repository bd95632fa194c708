"""Generate tests/golden/adaptor_ref.npz by running the REAL reference's ManoAdaptor on the CPU.

Runs only in the build container (needs /root/reference and its assets/mano/fhb_skel_centeridx{0,9}.pkl); the committed
.npz is data -- the weights the reference trained, seeded inputs and what the reference's class makes of them -- nothing
of the reference's source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adaptor.py

meshreg.models.meshregnet imports on the CPU with the absent third-party modules stubbed (libyana.camutils.project,
libyana.modelutils.freeze, manopth.manolayer, manopth.rodrigues_layer: none of them is touched by ManoAdaptor).

Recorded:
  adaptor_c0, adaptor_c9   [21,778] float32: key "adaptor" of the two pickles
  reordered_regressor      [21,778]: J_regressor of ManoAdaptor(layer, load_path=None) for an object whose ``_buffers`` holds
                           the th_J_regressor of SynthManoLayer() (the network's layer: 15 components, centre 9, seed 0)
  pose [3,18], betas [3,10]  seeded; verts_mm = SynthManoLayer().forward_torch(pose, betas)[0]; verts_m = verts_mm / 1000
  w_joints [3,21,3], w_verts [3,778,3]  the seeded linear functional  L = sum(w_joints * joints3d) + sum(w_verts * verts3d)
  per centre c in (9, 0), with ManoAdaptor(None, fhb_skel_centeridx{c}.pkl) and meshregnet.py:193-198's four lines:
    c{c}_adapt_joints [3,21,3], c{c}_joints3d [3,21,3], c{c}_verts3d [3,778,3], c{c}_grad_verts [3,778,3] = dL / d verts_m,
    c{c}_grad_weight [21,778] = dL / d adaptor.weight
"""
import os
import pickle
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.path.insert(0, REFERENCE)
sys.path.insert(0, ROOT)


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules.get(parent) or _stub(parent), leaf, mod)
    return mod


_stub("libyana.camutils.project")
_stub("libyana.modelutils.freeze", rec_freeze=lambda module: None)
_stub("manopth.manolayer", ManoLayer=object)
_stub("manopth.rodrigues_layer")  # (objbranch.py:3 wants the name from the package)

from meshreg.models.meshregnet import ManoAdaptor  # noqa: E402

from handobjectconsist_amd.models.synthnet import SynthManoLayer  # noqa: E402

CENTERS = (9, 0)
B = 3


class _Buffers:
    """all the reference's load_path=None branch reads of a MANO layer"""

    def __init__(self, regressor):
        self._buffers = {"th_J_regressor": regressor}


def main():
    torch.set_num_threads(1)
    out = {}
    paths = {c: os.path.join(REFERENCE, "assets", "mano", f"fhb_skel_centeridx{c}.pkl") for c in CENTERS}
    for c, path in paths.items():
        with open(path, "rb") as fh:
            out[f"adaptor_c{c}"] = np.ascontiguousarray(pickle.load(fh)["adaptor"], dtype=np.float32)
    layer = SynthManoLayer()
    out["reordered_regressor"] = ManoAdaptor(_Buffers(layer.th_J_regressor.clone())).J_regressor.numpy().copy()

    g = torch.Generator().manual_seed(20)
    pose = 0.4 * torch.randn(B, 18, generator=g)
    betas = torch.randn(B, 10, generator=g)
    w_joints = torch.randn(B, 21, 3, generator=g)
    w_verts = torch.randn(B, 778, 3, generator=g)
    with torch.no_grad():
        verts_mm = layer.forward_torch(pose, betas)[0]
    verts_m = verts_mm / 1000
    out.update(pose=pose.numpy(), betas=betas.numpy(), verts_mm=verts_mm.numpy(), verts_m=verts_m.numpy(), w_joints=w_joints.numpy(),
               w_verts=w_verts.numpy())
    for c in CENTERS:
        adaptor = ManoAdaptor(None, paths[c])
        assert adaptor.adaptor.weight.requires_grad
        verts3d = verts_m.clone().requires_grad_(True)
        # meshregnet.py:193-198, with mano_results["verts3d"] = verts3d and mano_center_idx = c
        adapt_joints, _ = adaptor(verts3d)
        adapt_joints = adapt_joints.transpose(1, 2)
        joints3d = adapt_joints - adapt_joints[:, c].unsqueeze(1)
        verts3d_c = verts3d - adapt_joints[:, c].unsqueeze(1)
        loss = (w_joints * joints3d).sum() + (w_verts * verts3d_c).sum()
        g_verts, g_weight = torch.autograd.grad(loss, [verts3d, adaptor.adaptor.weight])
        out[f"c{c}_adapt_joints"] = adapt_joints.detach().numpy().copy()
        out[f"c{c}_joints3d"] = joints3d.detach().numpy().copy()
        out[f"c{c}_verts3d"] = verts3d_c.detach().numpy().copy()
        out[f"c{c}_grad_verts"] = g_verts.numpy().copy()
        out[f"c{c}_grad_weight"] = g_weight.numpy().copy()
    for k, v in out.items():
        assert v.dtype == np.float32, k
    path = os.path.join(HERE, "adaptor_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ", ".join(f"{k}{list(v.shape)}" for k, v in out.items()))


if __name__ == "__main__":
    main()
