"""mr_jpeg_reconstruct (dequantisation + islow IDCT + fancy upsampling + YCbCr -> RGB of entropy-decoded JPEG frames on the
GPU), every byte compared for equality with what Pillow decoded from the same streams (tests/golden/jpeg_pil.npz, recorded
by tests/golden/make_golden_jpeg.py; the cases: tests/jpeg_ref.py), and end to end: ``HandObjSet(decode="device")`` +
``assemble_batch`` against the host decode."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "jpeg_pil.npz"))
NAMES = json.loads(str(GOLD["meta"]))["names"]
FILL = 0xA5


def raw_reconstruct(cuda, packed):
    """The C-ABI call on [N, bytes] packed frames with the output (and 64 bytes behind it) pre-filled with 0xA5."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import jpegdecode

    lib = _lib.load()
    width, height, comps, lh, lv = geom = jpegdecode.batch_geometry(packed)
    n = packed.shape[0]
    size = n * height * width * 3
    out = torch.full((size + 64,), FILL, dtype=torch.uint8, device=cuda)
    wbytes = int(lib.mr_jpeg_reconstruct_workspace_bytes(n, *geom))
    work = torch.full((wbytes + 64,), FILL, dtype=torch.uint8, device=cuda)
    packed_d = torch.from_numpy(packed).to(cuda)
    _lib.call("mr_jpeg_reconstruct", _lib.ptr(packed_d), n, width, height, comps, lh, lv, _lib.ptr(out), _lib.ptr(work), wbytes,
              _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert bool((out[size:] == FILL).all()) and bool((work[wbytes:] == FILL).all()), "wrote behind a buffer"
    return out[:size].cpu().numpy().reshape(n, height, width, 3)


@pytest.mark.parametrize("name", NAMES)
def test_matches_pillow_golden(cuda, name):
    from handobjectconsist_amd.datasets import jpegdecode

    packed = jpegdecode.entropy_decode(GOLD[name + "_stream"].tobytes())
    want = GOLD[name + "_rgb"]
    got = raw_reconstruct(cuda, packed[None])[0]
    assert got.shape == want.shape and int((got != want).sum()) == 0
    assert np.array_equal(jpegdecode.reconstruct(packed[None], cuda)[0].cpu().numpy(), want)


def test_a_batch_with_tables_per_frame(cuda):
    """Three 48 x 40 frames of different content and quality (their own quantisation tables) in one call."""
    from handobjectconsist_amd.datasets import jpegdecode

    packed = np.stack([jpegdecode.entropy_decode(GOLD[n + "_stream"].tobytes()) for n in R.BATCH])
    assert len({packed[k, 64:R.HEADER_BYTES].tobytes() for k in range(3)}) == 3
    want = np.stack([GOLD[n + "_rgb"] for n in R.BATCH])
    assert np.array_equal(raw_reconstruct(cuda, packed), want)
    got = jpegdecode.reconstruct(torch.from_numpy(packed), cuda)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (3, 40, 48, 3) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(jpegdecode.decode_batch([GOLD[n + "_stream"].tobytes() for n in R.BATCH], cuda).cpu().numpy(), want)


def test_odd_sizes_share_dwords_across_rows_and_frames(cuda):
    """37 x 29 frames: rows and frames start at bytes that are no multiple of 4, so a thread's four pixels straddle rows and
    frames; the last thread of the call owns fewer than four."""
    from handobjectconsist_amd.datasets import jpegdecode

    names = ("g37x29_s2", "optimize_37x29_s2", "rst1_37x29_s2", "rst2_37x29_s2", "q5_37x29_s2")
    packed = np.stack([jpegdecode.entropy_decode(GOLD[n + "_stream"].tobytes()) for n in names])
    assert (5 * 37 * 29) % 4 == 1
    assert np.array_equal(raw_reconstruct(cuda, packed), np.stack([GOLD[n + "_rgb"] for n in names]))


def test_no_frames(cuda):
    from handobjectconsist_amd import _lib

    out = torch.full((64,), FILL, dtype=torch.uint8, device=cuda)
    assert _lib.call("mr_jpeg_reconstruct", None, 0, 48, 40, 3, 2, 2, _lib.ptr(out), None, 0, _lib.stream_ptr(cuda)) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


def test_decode_batch_hands_unsupported_files_to_pillow_on_request(cuda):
    from handobjectconsist_amd.datasets import jpegdecode

    files = [GOLD["g48x40_s2_stream"].tobytes(), GOLD["progressive_stream"].tobytes(), GOLD["g48x40_s0_stream"].tobytes()]
    want = np.stack([GOLD["g48x40_s2_rgb"], GOLD["progressive_rgb"], GOLD["g48x40_s0_rgb"]])
    got = jpegdecode.decode_batch(files, cuda, unsupported="pillow")
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(jpegdecode.decode_batch(files, cuda, threads=1, unsupported="pillow").cpu().numpy(), want)
    with pytest.raises(NotImplementedError):
        jpegdecode.decode_batch(files, cuda)
    with pytest.raises(ValueError):
        jpegdecode.decode_batch(files[:1] + [GOLD["g37x29_s2_stream"].tobytes()], cuda)  # two frame sizes


@pytest.fixture(scope="module")
def dataset_batches():
    """B = 2 sequences of 2 frames of ``SynthPoseDataset(jpeg_quality=90)`` (272 x 248: partial MCUs at 4:2:0), once decoded
    by Pillow in the dataset and once carried as packed frames, on the same RNG streams; mirrored samples among them."""
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.utils import collate

    out = {}
    for decode in ("host", "device"):
        ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=(272, 248), seed=1, sides=("right", "left"), jpeg_quality=90)
        hs = handobjset.HandObjSet(ds, inp_res=(64, 64), color_fn="device", decode=decode, sample_nb=2, sides="right")
        random.seed(21)
        torch.manual_seed(21)
        out[decode] = collate.seq_extend_collate([hs[i] for i in (0, 3)], ["objverts3d", "objfaces", "objcanverts"])
    return out


@pytest.mark.parametrize("compact", [False, True], ids=["fp32", "compact"])
def test_dataset_device_decode_equals_host_decode(cuda, dataset_batches, compact):
    from handobjectconsist_amd.datasets import handobjset

    dtypes = dict(image_dtype=torch.bfloat16, mask_dtype=torch.uint8) if compact else {}
    host, dev = dataset_batches["host"], dataset_batches["device"]
    assert len(dev) == 2 and all(d["frame_jpeg"].dim() == 2 and d["frame_jpeg"].shape[0] == 2 and "frame" not in d for d in dev)
    assert any(bool(d["flip"].any()) for d in dev) and not all(bool(d["flip"].all()) for d in dev)
    a = handobjset.assemble_batch(host, cuda, (64, 64), **dtypes)
    b = handobjset.assemble_batch(dev, cuda, (64, 64), **dtypes)
    for fa, fb in zip(a, b):
        assert "frame_jpeg" not in fb and fa.keys() == fb.keys()
        assert fa["image"].dtype == fb["image"].dtype and fa["image"].shape == (2, 3, 64, 64) and torch.equal(fa["image"], fb["image"])
        assert fa["jittermask"].dtype == fb["jittermask"].dtype and torch.equal(fa["jittermask"], fb["jittermask"])
        assert float(fa["jittermask"].float().mean()) > 0.2, "the crops miss the frames"
