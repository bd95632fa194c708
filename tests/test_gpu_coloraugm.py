"""mr_frames_color_augment (Gaussian blur + colour jitter of decoded frames on the GPU) through the C-ABI, every byte
compared for equality: against tests/golden/coloraugm_pil.npz (the real Pillow, mirrored samples among them), against the
numpy checker tests/coloraugm_ref.py (itself pinned to Pillow by tests/test_oracle_coloraugm.py) on shapes around the
kernels' boundaries, and end to end -- ``HandObjSet(color_fn="device")`` + ``assemble_batch`` against the host path."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import coloraugm_ref as C
from tests import dataset_fake

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "coloraugm_pil.npz"))
META = json.loads(str(GOLD["meta"]))


def augment(cuda, frames, plans, flip=None):
    from handobjectconsist_amd.datasets import frames as F

    return F.color_augment(torch.from_numpy(np.ascontiguousarray(frames)).to(cuda), plans, flip=flip).cpu().numpy()


def plan_ops(plan):
    return [(int(c), v) for c, v in zip(plan[1:5], plan[5:9]) if int(c) != C.OP_NONE]


def make_plan(radius, ops):
    plan = np.zeros(9, np.float32)
    plan[0] = radius
    for k, (code, value) in enumerate(ops):
        plan[1 + k], plan[5 + k] = code, value
    return plan


def random_ops(rng):
    codes = rng.permutation([C.OP_BRIGHTNESS, C.OP_SATURATION, C.OP_HUE, C.OP_CONTRAST])[: int(rng.integers(0, 5))]
    return [(int(c), float(rng.integers(-127, 128)) if c == C.OP_HUE else float(np.float32(rng.uniform(0, 2)))) for c in codes]


@pytest.mark.parametrize("case", range(META["cases"]))
def test_matches_pillow_golden(cuda, case):
    got = augment(cuda, GOLD[f"c{case}_in"], GOLD[f"c{case}_plan"], flip=GOLD[f"c{case}_flip"])
    assert np.array_equal(got, GOLD[f"c{case}_out"])


def test_random_cases_match_the_checker(cuda):
    """200 cases: widths that are no multiple of 4 and sit around a wave (63, 64, 65) and past a strip (257), heights 1, 2 and
    130 (more than one run of a column, more than one block of rows), radius 0, box radii above the width, 0 to 4 ops."""
    rng = np.random.default_rng(7)
    widths, heights = [3, 5, 63, 64, 65, 257], [1, 2, 130]
    for trial in range(200):
        w, h = widths[trial % 6], heights[(trial // 6) % 3]
        radius = [0.0, float(rng.uniform(0, 1)), float(rng.uniform(1, 6)), float(rng.uniform(1.5, 2.5)) * w][trial % 4]
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if trial % 5 == 0:
            frame[...] = frame[..., :1]  # grey frames: S = 0
        plan = make_plan(radius, random_ops(rng))
        if trial % 4 == 3:
            assert C.box_weights(C.box_radius(plan[0]))[0] > w
        want = C.apply_plan(frame, plan[0], plan_ops(plan))
        got = augment(cuda, frame[None], plan[None], flip=[trial % 2])[0]
        assert np.array_equal(got, want), (trial, w, h, plan)


def test_hue_on_every_colour(cuda):
    """The hue op alone on all 2^24 colours (a 4096 x 4096 frame), three shifts."""
    cube = C.color_cube()
    hsv = C.rgb_to_hsv(cube).astype(np.int32)
    table = C.hsv_to_rgb(cube).reshape(-1, 3)  # HSV triple (as the cube indexes it) -> RGB
    for shift in (-127, 38, 101):
        want = table[(((hsv[..., 0] + shift) & 255) << 16) | (hsv[..., 1] << 8) | hsv[..., 2]]
        got = augment(cuda, cube[None], make_plan(0.0, [(C.OP_HUE, shift)])[None])[0]
        assert np.array_equal(got, want), shift


def test_a_batch_with_a_plan_per_frame(cuda):
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (6, 41, 29, 3), dtype=np.uint8)
    plans = np.stack([make_plan([0.0, 0.2, 0.5, 1.1, 3.0, 0.35][n], random_ops(rng)) for n in range(6)])
    plans[2] = make_plan(0.5, [(C.OP_SATURATION, 1.4), (C.OP_CONTRAST, 0.6), (C.OP_HUE, -30), (C.OP_BRIGHTNESS, 1.2)])
    plans[4, 1:] = 0
    got = augment(cuda, frames, plans, flip=[0, 1, 0, 1, 1, 0])
    for n in range(6):
        assert np.array_equal(got[n], C.apply_plan(frames[n], plans[n, 0], plan_ops(plans[n]))), n
    # ... and again: nothing depends on the order the workgroups arrive in
    assert np.array_equal(augment(cuda, frames, plans), got)


def _raw(cuda, frames, radius, codes, values, n=None, h=None, w=None, in_off=0, out_off=0, work_off=0, work_short=0, flip=None):
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    N, H, W = frames.shape[:3]
    n, h, w = N if n is None else n, H if h is None else h, W if w is None else w
    src = torch.zeros(frames.size + 16, dtype=torch.uint8, device=cuda)
    src[: frames.size] = torch.from_numpy(frames.reshape(-1)).to(cuda)
    dst = torch.zeros_like(src)
    wbytes = max(int(lib.mr_frames_color_augment_workspace_bytes(N, H, W)), 16)
    work = torch.empty(wbytes + 16, dtype=torch.uint8, device=cuda)
    radius, values = np.asarray(radius, np.float32), np.asarray(values, np.float32)
    codes = np.asarray(codes, np.int32)
    rc = lib.mr_frames_color_augment(src.data_ptr() + in_off, dst.data_ptr() + out_off, None if flip is None else flip.ctypes.data,
                                     radius.ctypes.data, codes.ctypes.data, values.ctypes.data, work.data_ptr() + work_off,
                                     wbytes - work_short, n, h, w, _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    return rc, dst[: frames.size].cpu().numpy().reshape(frames.shape)


def test_empty_batches_and_bad_arguments(cuda):
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    frames = np.random.default_rng(9).integers(0, 256, (2, 6, 5, 3), dtype=np.uint8)
    ok = dict(radius=[0.5, 0.0], codes=[[1, 3, 0, 4], [0, 0, 0, 0]], values=[[1.2, -127, 0, 0.5], [0, 0, 0, 0]])
    rc, out = _raw(cuda, frames, **ok)
    assert rc == 0
    for n in range(2):
        plan = make_plan(ok["radius"][n], [(c, v) for c, v in zip(ok["codes"][n], ok["values"][n]) if c])
        assert np.array_equal(out[n], C.apply_plan(frames[n], plan[0], plan_ops(plan)))
    for empty in (dict(n=0), dict(h=0), dict(w=0)):
        rc, out = _raw(cuda, frames, **ok, **empty)
        assert rc == 0 and not out.any()
    assert augment(cuda, np.zeros((0, 4, 4, 3), np.uint8), np.zeros((0, 9), np.float32)).shape == (0, 4, 4, 3)
    assert lib.mr_frames_color_augment_workspace_bytes(-1, 4, 4) == -1

    def bad(**change):
        rc, out = _raw(cuda, frames, **{**ok, **change})
        assert not out.any(), change  # refused before any launch
        return rc

    assert bad(codes=[[1, 5, 0, 0], [0] * 4]) == -1  # unknown op
    assert bad(codes=[[-1, 0, 0, 0], [0] * 4]) == -1
    assert bad(codes=[[1, 1, 0, 0], [0] * 4]) == -1  # an op twice
    assert bad(values=[[np.nan, 0, 0, 0.5], [0] * 4]) == -1  # non-finite factor
    assert bad(values=[[1.2, 0, 0, np.inf], [0] * 4]) == -1
    assert bad(values=[[1.2, 128, 0, 0.5], [0] * 4]) == -1  # hue shift outside +-127
    assert bad(values=[[1.2, -128, 0, 0.5], [0] * 4]) == -1
    assert bad(values=[[1.2, 3.5, 0, 0.5], [0] * 4]) == -1  # ... or no integer
    assert bad(radius=[-0.5, 0.0]) == -1
    assert bad(radius=[np.nan, 0.0]) == -1
    assert bad(n=-1) == -1
    assert bad(in_off=1) == -1 and bad(out_off=2) == -1 and bad(work_off=8) == -1  # misaligned pointers
    assert bad(work_short=1) == -1
    assert bad(h=10753, work_short=-(1 << 40)) == -2  # a column no longer fits a workgroup's LDS
    assert bad(n=65536, work_short=-(1 << 40)) == -2  # a frame is a grid row
    null = ctypes.c_void_p(None)
    assert lib.mr_frames_color_augment(null, null, null, null, null, null, null, 0, 1, 4, 4, None) == -1


def test_python_layer_refuses_what_it_cannot_mean(cuda):
    from handobjectconsist_amd.datasets import handobjset

    frames = np.zeros((2, 4, 4, 3), np.uint8)
    plans = np.stack([make_plan(0.5, [(C.OP_BRIGHTNESS, 1.2)]), make_plan(0.0, [])])
    plans[0, 1] = 1.5  # an op code that is no integer: not op 1
    with pytest.raises(ValueError, match="op codes"):
        augment(cuda, frames, plans)
    plans[0, 1] = np.nan
    with pytest.raises(ValueError, match="op codes"):
        augment(cuda, frames, plans)
    one = dict(frame=torch.zeros(1, 4, 4, 3, dtype=torch.uint8), affinetrans=np.eye(3)[None], flip=np.zeros(1, bool))
    mixed = [dict(one, color_plan=make_plan(0.0, [])[None]), dict(one)]
    with pytest.raises(ValueError, match="color_plan in 1 of 2"):
        handobjset.assemble_batch(mixed, cuda, (4, 4))


def test_in_place(cuda):
    """frames_in == frames_out is allowed."""
    from handobjectconsist_amd import _lib

    rng = np.random.default_rng(10)
    frames = rng.integers(0, 256, (3, 19, 70, 3), dtype=np.uint8)
    plans = np.stack([make_plan(r, random_ops(rng)) for r in (0.0, 0.5, 2.0)])
    buf = torch.from_numpy(frames).to(cuda)
    lib = _lib.load()
    wbytes = int(lib.mr_frames_color_augment_workspace_bytes(3, 19, 70))
    work = torch.empty(wbytes, dtype=torch.uint8, device=cuda)
    radius, codes, values = plans[:, 0].copy(), plans[:, 1:5].astype(np.int32), plans[:, 5:9].copy()
    _lib.call("mr_frames_color_augment", _lib.ptr(buf), _lib.ptr(buf), None, radius.ctypes.data, codes.ctypes.data,
              values.ctypes.data, _lib.ptr(work), wbytes, 3, 19, 70, _lib.stream_ptr(cuda))
    assert np.array_equal(buf.cpu().numpy(), augment(cuda, frames, plans))


@pytest.fixture(scope="module")
def dataset_batches():
    """Collated batches of the pair and the triple configuration of tests/dataset_fake.py (sides 'right' / 'left': mirrored
    hands among the samples), once through the host path and once through the device path, on the same RNG streams."""
    from handobjectconsist_amd.datasets import handobjset
    from handobjectconsist_amd.utils import collate

    out = {}
    for cname, kw, seed, idxs in dataset_fake.CONFIGS:
        if cname not in ("train_pair_right", "train_triple_left_blockrot", "train_pair_blur"):
            continue
        for mode in ("reference", "device"):
            ds = dataset_fake.FakePoseDataset(pil=False)
            hs = handobjset.HandObjSet(ds, inp_res=dataset_fake.INP_RES, color_fn=mode, **{"train": True, **kw})
            random.seed(seed)
            torch.manual_seed(seed)
            out[cname, mode] = collate.seq_extend_collate([hs[i] for i in idxs], ["objverts3d", "objfaces", "objcanverts"])
    return out


@pytest.mark.parametrize("compact", [False, True], ids=["fp32", "compact"])
@pytest.mark.parametrize("cname", ["train_pair_right", "train_triple_left_blockrot", "train_pair_blur"])
def test_dataset_device_path_equals_host_path(cuda, dataset_batches, cname, compact):
    from handobjectconsist_amd.datasets import handobjset

    dtypes = dict(image_dtype=torch.bfloat16, mask_dtype=torch.uint8) if compact else {}
    host, dev = dataset_batches[cname, "reference"], dataset_batches[cname, "device"]
    assert all("color_plan" in d and d["color_plan"].shape == (len(d["frame"]), 9) for d in dev)
    assert any(bool(d["flip"].any()) for d in dev), "no mirrored sample in the batch"
    assert any(not torch.equal(h["frame"], d["frame"]) for h, d in zip(host, dev)), "the host path changed no frame"
    a = handobjset.assemble_batch(host, cuda, dataset_fake.INP_RES, **dtypes)
    b = handobjset.assemble_batch(dev, cuda, dataset_fake.INP_RES, **dtypes)
    for fa, fb in zip(a, b):
        assert "color_plan" not in fb and fa.keys() == fb.keys()
        assert fa["image"].dtype == fb["image"].dtype and torch.equal(fa["image"], fb["image"])
        assert fa["jittermask"].dtype == fb["jittermask"].dtype and torch.equal(fa["jittermask"], fb["jittermask"])
