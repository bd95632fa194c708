"""Generate tests/golden/chain_dataset2d.npz by RUNNING THE REFERENCE'S OWN dataset glue on CPU with the 2-D queries.

Build container only (needs the reference checkout ``make_golden_dataset.py`` names).  The committed .npz is data: seeded inputs' outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dataset2d.py

``make_golden_dataset.py``'s arrangement and its stubs, taken from that file as they are (``install()``): the reference's
``HandObjSet.get_sample`` / ``__getitem__`` (meshreg/datasets/handobjset.py:93-430) and ``seq_extend_collate`` run unmodified around
tests/dataset_fake2d.FakePoseDataset2d, on the same configurations and seeds, with that generator's queries PLUS
BaseQueries / TransQueries JOINTS2D, OBJVERTS2D and HANDVERTS2D (handobjset.py:160-225); the collate pads OBJVERTS2D of both
enums beside the three 3-D entries, as trainmeshwarp.py's ``extend_queries`` do.  Stored: per sample the affine and the six 2-D
arrays as the reference returned them (dtype included: it leaves HANDVERTS2D's transformed array in float64), per collated dict
the affine and the joints' and object's arrays, and per configuration the augmentation drawn for the first index and where the
random stream stands after the items -- both equal chain_dataset.npz's: the 2-D queries draw nothing."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_dataset", os.path.join(HERE, "make_golden_dataset.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
from tests import dataset_fake2d  # noqa: E402


def main():
    handobjset, collate, Q = base.install()
    B, T = Q.BaseQueries, Q.TransQueries
    queries = [T.IMAGE, T.JITTERMASK, T.AFFINETRANS, T.CAMINTR, B.CAMINTR, T.JOINTS3D, B.JOINTS3D, T.HANDVERTS3D, T.OBJVERTS3D,
               B.OBJFACES, B.OBJCANVERTS, B.SIDE, B.JOINTS2D, T.JOINTS2D, B.OBJVERTS2D, T.OBJVERTS2D, B.HANDVERTS2D, T.HANDVERTS2D]
    names = {T.AFFINETRANS: "affinetrans", B.JOINTS2D: "joints2d", T.JOINTS2D: "joints2d_trans", B.OBJVERTS2D: "objverts2d",
             T.OBJVERTS2D: "objverts2d_trans", B.HANDVERTS2D: "handverts2d", T.HANDVERTS2D: "handverts2d_trans", T.OBJVERTS3D: "objverts3d"}
    collated = ("affinetrans", "joints2d", "joints2d_trans", "objverts2d", "objverts2d_trans")
    old = np.load(os.path.join(HERE, "chain_dataset.npz"))
    arrays, meta = {}, {"configs": {}, "inp_res": list(dataset_fake2d.INP_RES)}
    for cname, kw, seed, idxs in dataset_fake2d.CONFIGS:
        ds = dataset_fake2d.FakePoseDataset2d(pil=True)
        hs = handobjset.HandObjSet(ds, inp_res=dataset_fake2d.INP_RES, queries=queries, **{"train": True, "blur_radius": 0.0, **kw})
        torch.manual_seed(seed)
        sa = hs.get_sample(idxs[0])["space_augm"]
        arrays[f"{cname}/space_center"] = np.asarray(sa["center"], np.float64)
        arrays[f"{cname}/space_scale_rot"] = np.asarray([sa["scale"], sa["rot"]], np.float64)
        torch.manual_seed(seed)
        items = [hs[i] for i in idxs]
        arrays[f"{cname}/rng_after"] = torch.rand(4).numpy()
        for key in ("space_center", "space_scale_rot", "rng_after"):
            assert np.array_equal(arrays[f"{cname}/{key}"], old[f"{cname}/{key}"]), (cname, key)
        for n, item in enumerate(items):
            for k, sample in enumerate(item if isinstance(item, list) else [item]):
                for key, name in names.items():
                    if name != "objverts3d":
                        arrays[f"{cname}/item{n}/frame{k}/{name}"] = np.asarray(sample[key])
        meta["configs"][cname] = {"idxs": idxs, "seed": seed, "frames_per_item": len(items[0]) if isinstance(items[0], list) else 1}
        torch.manual_seed(seed)
        items = [hs[i] for i in idxs]
        ext = [T.OBJVERTS3D, B.OBJFACES, B.OBJCANVERTS, B.OBJVERTS2D, T.OBJVERTS2D]
        batch = collate.seq_extend_collate(items, ext) if isinstance(items[0], list) else [collate.extend_collate(items, ext)]
        for k, frame in enumerate(batch):
            for key, name in names.items():
                if name in collated:
                    arrays[f"{cname}/collated/frame{k}/{name}"] = frame[key].numpy()
                    meta["configs"][cname].setdefault("collated_dtypes", {})[name] = str(frame[key].dtype)
            meta["configs"][cname].setdefault("collated_objverts3d_rows", []).append(int(frame[T.OBJVERTS3D].shape[1]))
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "chain_dataset2d.npz")
    np.savez_compressed(path, **arrays)
    print(f"chain_dataset2d.npz: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
