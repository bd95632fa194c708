"""mr_png_unfilter (the PNG row filters undone on the GPU, alpha dropped, grey replicated), every byte compared for equality
with what Pillow decoded from the same streams (tests/golden/png_pil.npz, recorded by tests/golden/make_golden_png.py; the
cases: tests/png_ref.py), and end to end: ``HandObjSet(decode="device")`` on PNG bytes + ``assemble_batch`` against the host
decode."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import png_ref as R

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "png_pil.npz"))
NAMES = json.loads(str(GOLD["meta"]))["names"]
FILL = 0xA5


def raw_unfilter(cuda, packed):
    """The C-ABI call on [N, bytes] packed frames with the output pre-filled with 0xA5 and sized one guard row beyond."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import pngdecode

    width, height, channels = pngdecode.batch_geometry(packed)
    n = packed.shape[0]
    size = n * height * width * 3
    guard = max(width * 3, 64)
    out = torch.full((size + guard,), FILL, dtype=torch.uint8, device=cuda)
    packed_d = torch.from_numpy(packed).to(cuda)
    _lib.call("mr_png_unfilter", _lib.ptr(packed_d), n, width, height, channels, _lib.ptr(out), None, _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert bool((out[size:] == FILL).all()), "wrote behind the frames"
    return out[:size].cpu().numpy().reshape(n, height, width, 3)


@pytest.mark.parametrize("name", NAMES)
def test_matches_pillow_golden(cuda, name):
    from handobjectconsist_amd.datasets import pngdecode

    packed = pngdecode.inflate(GOLD[name + "_stream"].tobytes())
    want = GOLD[name + "_rgb"]
    got = raw_unfilter(cuda, packed[None])[0]
    assert got.shape == want.shape and int((got != want).sum()) == 0
    assert np.array_equal(pngdecode.unfilter(packed[None], cuda)[0].cpu().numpy(), want)


def test_the_golden_cases_are_the_ones_the_kernel_can_go_wrong_at():
    from handobjectconsist_amd import _lib

    assert R.BAND_ROWS == _lib.PNG_BAND_ROWS and f"h{2 * _lib.PNG_BAND_ROWS + 3}_w3" in NAMES
    for name in ("tiny1x1_c3", "tiny1x9_c1", "tiny9x1_c4", "f43120_5x7_c2", "first_paeth_6x4", "first_average_6x4", "first_up_6x4",
                 "paeth_ties_c1", "average_carry", "h63_w5", "h64_w5", "h65_w5", "h257_w5", "w1_h6_c1", "w3_h6_c2", "w4_h6_c3",
                 "w5_h6_c4", "w67_h6_c3", "pil48x40_c2"):
        assert name in NAMES, name


def test_a_batch_with_filters_per_frame(cuda):
    """Three 37 x 29 frames of different content and different row filters in one call; rows and frames start at bytes that
    are no multiple of 4."""
    from handobjectconsist_amd.datasets import pngdecode

    packed = np.stack([pngdecode.inflate(GOLD[n + "_stream"].tobytes()) for n in R.BATCH])
    stride = 1 + 37 * 3
    assert len({packed[k, 64:64 + 29 * stride:stride].tobytes() for k in range(3)}) == 3 and (37 * 29 * 3) % 4 == 3
    want = np.stack([GOLD[n + "_rgb"] for n in R.BATCH])
    assert np.array_equal(raw_unfilter(cuda, packed), want)
    got = pngdecode.unfilter(torch.from_numpy(packed), cuda)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (3, 29, 37, 3) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(pngdecode.decode_batch([GOLD[n + "_stream"].tobytes() for n in R.BATCH], cuda).cpu().numpy(), want)


def test_a_batch_of_dword_aligned_frames(cuda):
    """Four 48 x 40 RGB frames (widths that are a multiple of 4 store whole dwords), one of them twice."""
    from handobjectconsist_amd.datasets import pngdecode

    names = ("pil48x40_c3", "pil_optimize", "pil48x40_c3", "pil_optimize")
    packed = np.stack([pngdecode.inflate(GOLD[n + "_stream"].tobytes()) for n in names])
    assert np.array_equal(raw_unfilter(cuda, packed), np.stack([GOLD[n + "_rgb"] for n in names]))


def test_no_frames(cuda):
    from handobjectconsist_amd import _lib

    out = torch.full((64,), FILL, dtype=torch.uint8, device=cuda)
    assert _lib.call("mr_png_unfilter", None, 0, 48, 40, 3, _lib.ptr(out), None, _lib.stream_ptr(cuda)) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


def test_decode_batch_hands_unsupported_files_to_pillow_on_request(cuda):
    from handobjectconsist_amd.datasets import pngdecode

    files = [GOLD[R.BATCH[0] + "_stream"].tobytes(), GOLD["palette_stream"].tobytes(), GOLD[R.BATCH[2] + "_stream"].tobytes()]
    want = np.stack([GOLD[R.BATCH[0] + "_rgb"], GOLD["palette_rgb"], GOLD[R.BATCH[2] + "_rgb"]])
    got = pngdecode.decode_batch(files, cuda, unsupported="pillow")
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(pngdecode.decode_batch(files, cuda, threads=1, unsupported="pillow").cpu().numpy(), want)
    with pytest.raises(NotImplementedError):
        pngdecode.decode_batch(files, cuda)
    with pytest.raises(ValueError):
        pngdecode.decode_batch(files[:1] + [GOLD["pil48x40_c3_stream"].tobytes()], cuda)  # two frame sizes



def test_decode_batch_groups_interleaved_geometries_of_one_frame_size(cuda):
    """Five 48 x 40 files of 3, 4, 1, 3 and 2 channels: four geometries of one frame size, so ``decode_batch`` unfilters four
    groups of packed frames (one of them of two files that are not neighbours) and puts the frames back in the files' order."""
    from handobjectconsist_amd.datasets import pngdecode

    names = ("pil48x40_c3", "pil48x40_c4", "pil48x40_c1", "pil48x40_c3", "pil48x40_c2")
    files = [GOLD[n + "_stream"].tobytes() for n in names]
    assert len({pngdecode.inflate(f)[:16].tobytes() for f in files}) == 4
    want = np.stack([GOLD[n + "_rgb"] for n in names])
    got = pngdecode.decode_batch(files, cuda)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (5, 40, 48, 3) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(pngdecode.decode_batch(files, cuda, threads=1).cpu().numpy(), want)


@pytest.fixture(scope="module")
def dataset_batches():
    """B = 2 sequences of 2 frames of ``SynthPoseDataset(png_compress_level=1)`` (272 x 248: four bands, the last partial),
    once decoded by Pillow in the dataset and once carried as packed frames, on the same RNG streams, with the colour
    augmentation on the device and without; mirrored samples among them."""
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.utils import collate

    out = {}
    for color_fn in ("device", None):
        for decode in ("host", "device"):
            ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=(272, 248), seed=1, sides=("right", "left"), png_compress_level=1)
            hs = handobjset.HandObjSet(ds, inp_res=(64, 64), color_fn=color_fn, decode=decode, sample_nb=2, sides="right")
            random.seed(21)
            torch.manual_seed(21)
            out[color_fn, decode] = collate.seq_extend_collate([hs[i] for i in (0, 3)], ["objverts3d", "objfaces", "objcanverts"])
    return out


@pytest.mark.parametrize("color_fn", ["device", None], ids=["color_device", "color_none"])
@pytest.mark.parametrize("compact", [False, True], ids=["fp32", "compact"])
def test_dataset_device_decode_equals_host_decode(cuda, dataset_batches, compact, color_fn):
    from handobjectconsist_amd.datasets import handobjset

    dtypes = dict(image_dtype=torch.bfloat16, mask_dtype=torch.uint8) if compact else {}
    host, dev = dataset_batches[color_fn, "host"], dataset_batches[color_fn, "device"]
    assert len(dev) == 2 and all(d["frame_png"].dim() == 2 and d["frame_png"].shape[0] == 2 and "frame" not in d for d in dev)
    assert all(("color_plan" in d) == (color_fn == "device") for d in dev)
    assert any(bool(d["flip"].any()) for d in dev) and not all(bool(d["flip"].all()) for d in dev)
    a = handobjset.assemble_batch(host, cuda, (64, 64), **dtypes)
    b = handobjset.assemble_batch(dev, cuda, (64, 64), **dtypes)
    for fa, fb in zip(a, b):
        assert "frame_png" not in fb and fa.keys() == fb.keys()
        assert fa["image"].dtype == fb["image"].dtype and fa["image"].shape == (2, 3, 64, 64) and torch.equal(fa["image"], fb["image"])
        assert fa["jittermask"].dtype == fb["jittermask"].dtype and torch.equal(fa["jittermask"], fb["jittermask"])
        assert float(fa["jittermask"].float().mean()) > 0.2, "the crops miss the frames"
