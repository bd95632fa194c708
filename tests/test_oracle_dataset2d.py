"""The 2-D queries of the dataset glue pinned by RUNNING the reference: tests/golden/chain_dataset2d.npz holds what
the reference's ``HandObjSet.get_sample`` / ``__getitem__`` (meshreg/datasets/handobjset.py:160-225) and ``seq_extend_collate``
returned for BaseQueries / TransQueries JOINTS2D, OBJVERTS2D, HANDVERTS2D and TransQueries.AFFINETRANS around
tests/dataset_fake2d.FakePoseDataset2d, on tests/dataset_fake.CONFIGS' configurations and seeds (generator:
tests/golden/make_golden_dataset2d.py, stubbed as make_golden_dataset.py is).  The package's host path must reproduce it with
tests/test_oracle_dataset.py's rule for float entries -- ``np.array_equal``, bit for bit --: the mirror ``W - x``, the transform of
the array as the accessor returned it (float64 joints), float32 results (the reference leaves HANDVERTS2D's transformed array in
float64: its values cast once), the cyclic padding of ``objverts2d`` in step with ``objverts3d``; and the 2-D queries draw nothing:
the augmentation and the random stream's position are chain_dataset.npz's."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dataset_fake2d

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chain_dataset2d.npz")
QUERIES = ("frame", "camintr", "joints3d", "handverts3d", "objverts3d", "objfaces", "objcanverts", "side", "affinetrans", "joints2d",
           "joints2d_trans", "objverts2d", "objverts2d_trans", "handverts2d", "handverts2d_trans")
NAMES = QUERIES[9:]


def build(kw):
    from handobjectconsist_amd.datasets import coloraugm, handobjset

    ds = dataset_fake2d.FakePoseDataset2d(pil=False)
    return ds, handobjset.HandObjSet(ds, inp_res=dataset_fake2d.INP_RES, queries=QUERIES, color_fn=coloraugm.make_color_fn(jitter=False),
                                   **{"train": True, "blur_radius": 0.0, **kw})


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["meta"])), np.load(os.path.join(HERE, "golden", "chain_dataset.npz"))


configs = pytest.mark.parametrize("cname,kw,seed,idxs", dataset_fake2d.CONFIGS, ids=[c[0] for c in dataset_fake2d.CONFIGS])


@configs
def test_samples_match_the_reference_run(golden, cname, kw, seed, idxs):
    g, meta, old = golden
    ds, hs = build(kw)
    torch.manual_seed(seed)
    first = hs.get_sample(idxs[0])
    for fixture in (g, old):  # the draws are those of the run without the 2-D queries
        assert np.array_equal(np.asarray(first["space_augm"]["center"], np.float64), fixture[f"{cname}/space_center"])
        assert np.array_equal(np.asarray([first["space_augm"]["scale"], first["space_augm"]["rot"]], np.float64), fixture[f"{cname}/space_scale_rot"])
    torch.manual_seed(seed)
    items = [hs[i] for i in idxs]
    after = torch.rand(4).numpy()
    assert np.array_equal(after, g[f"{cname}/rng_after"]) and np.array_equal(after, old[f"{cname}/rng_after"]), "RNG stream position after the items"
    mirrored = 0
    for n, item in enumerate(items):
        frames = item if isinstance(item, list) else [item]
        assert len(frames) == meta["configs"][cname]["frames_per_item"]
        for k, sample in enumerate(frames):
            ref = lambda name: g[f"{cname}/item{n}/frame{k}/{name}"]  # noqa: E731
            assert np.array_equal(sample["affinetrans"], ref("affinetrans")) and sample["affinetrans"].dtype == ref("affinetrans").dtype == np.float32
            for name in NAMES:
                assert sample[name].dtype == np.float32 and sample[name].shape == ref(name).shape, name
                assert np.array_equal(sample[name], ref(name).astype(np.float32)), name
            assert len(sample["objverts2d"]) == len(sample["objverts3d"]) and sample["joints2d"].shape == (21, 2)
            mirrored += bool(sample["flip"])
    if kw["sides"] != "both":
        assert 0 < mirrored < sum(len(i) if isinstance(i, list) else 1 for i in items), "the configuration mirrors some hands and not others"


@configs
def test_collated_batch_matches_the_reference_run(golden, cname, kw, seed, idxs):
    from handobjectconsist_amd.utils import collate

    g, meta, _ = golden
    info = meta["configs"][cname]
    ds, hs = build(kw)
    torch.manual_seed(seed)
    items = [hs[i] for i in idxs]
    batch = collate.seq_extend_collate(items, collate.EXTEND_QUERIES) if isinstance(items[0], list) else [collate.extend_collate(items, collate.EXTEND_QUERIES)]
    assert len(batch) == info["frames_per_item"]
    for k, frame in enumerate(batch):
        for name in ("affinetrans", "joints2d", "joints2d_trans", "objverts2d", "objverts2d_trans"):
            ref, got = g[f"{cname}/collated/frame{k}/{name}"], frame[name]
            assert torch.is_tensor(got) and str(got.dtype) == info["collated_dtypes"][name] == "torch.float32", (name, got.dtype)
            assert tuple(got.shape) == ref.shape and np.array_equal(got.numpy(), ref), name
        rows = info["collated_objverts3d_rows"][k]
        assert frame["objverts2d"].shape[1] == frame["objverts2d_trans"].shape[1] == frame["objverts3d"].shape[1] == rows
