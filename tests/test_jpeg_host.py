"""The host side of the device JPEG decode, without a GPU: what the entropy decoder refuses and how, the packed frame's
size, ``HandObjSet(decode="device")``'s samples against ``decode="host"``'s (same draws, same RNG streams afterwards),
``assemble_batch``'s and ``mr_jpeg_reconstruct``'s argument checks, and the stand-alone sanitizer program of
csrc/jpeg_entropy.hpp (tests/jpeg_entropy_main.cpp: a separate executable, nothing is loaded into the interpreter)."""
import ctypes
import io
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))


def _save(img, **opts):
    buf = io.BytesIO()
    img.save(buf, "JPEG", **opts)
    return buf.getvalue()


def test_unsupported_streams_raise_not_implemented():
    from handobjectconsist_amd.datasets import jpegdecode

    rgb = Image.fromarray(R.content(37, 29, 1))
    for data in (_save(rgb, quality=75, progressive=True), _save(rgb.convert("CMYK"), quality=75), GOLD["progressive_stream"].tobytes()):
        with pytest.raises(NotImplementedError):
            jpegdecode.entropy_decode(data)
        with pytest.raises(NotImplementedError):
            jpegdecode.jpeg_info(data)
    # other sampling factors (Pillow writes none): 4:1:1 (luma 4x1), 4:4:0 (luma 1x2), subsampled Cb -- decided from the
    # headers alone, so rewriting the factors in the frame header is enough
    good = bytearray(GOLD["g17x9_s2_stream"].tobytes())
    sof = bytes(good).index(b"\xff\xc0")
    assert good[sof + 11] == 0x22 and good[sof + 14] == 0x11
    for at, factors in ((11, 0x41), (11, 0x12), (14, 0x21)):
        bad = bytearray(good)
        bad[sof + at] = factors
        with pytest.raises(NotImplementedError):
            jpegdecode.entropy_decode(bytes(bad))
    twelve = bytearray(good)
    twelve[sof + 4] = 12
    with pytest.raises(NotImplementedError):
        jpegdecode.jpeg_info(bytes(twelve))


def test_malformed_streams_raise_value_error():
    from handobjectconsist_amd.datasets import jpegdecode

    good = GOLD["g17x9_s2_stream"].tobytes()
    rng = np.random.default_rng(3)
    sos = good.index(b"\xff\xda")
    streams = (b"", b"\xff", b"\xff\xd8", rng.integers(0, 256, 500, dtype=np.uint8).tobytes(), b"\x00" * 64, good[1:], good[:sos],
               good[:sos + 14], good[:len(good) // 2 + sos // 2], good[:sos + 16] + b"\xff\xd9")
    for k, data in enumerate(streams):
        with pytest.raises(ValueError):
            jpegdecode.entropy_decode(data)
        if k < 7:  # (the later ones have whole headers: jpeg_info reads no further)
            with pytest.raises(ValueError):
                jpegdecode.jpeg_info(data)
    assert jpegdecode.jpeg_info(streams[7])["width"] == 17
    # a restart marker with the wrong number, and one missing
    rst = bytearray(GOLD["rst1_37x29_s2_stream"].tobytes())
    at = bytes(rst).index(b"\xff\xd1")
    rst[at + 1] = 0xD3
    with pytest.raises(ValueError):
        jpegdecode.entropy_decode(bytes(rst))
    # coefficients whose product with their quantiser leaves 16 bits (here: quality-100 coefficients under quantisers of
    # 255) are outside what an encoder of 8-bit samples writes and outside the device IDCT's 32-bit contract: refused
    big = bytearray(GOLD["q100_37x29_s0_stream"].tobytes())
    dqt = bytes(big).index(b"\xff\xdb")
    assert big[dqt + 4] == 0 and set(big[dqt + 5:dqt + 69]) == {1}
    big[dqt + 5:dqt + 69] = bytes([255]) * 64
    with pytest.raises(ValueError):
        jpegdecode.entropy_decode(bytes(big))
    big[dqt + 5:dqt + 69] = bytes([16]) * 64  # ... while 16 x the same coefficients (at most about 1000) passes
    assert jpegdecode.entropy_decode(bytes(big)).size == jpegdecode.packed_bytes(37, 29, 3, 1, 1)
    # complete entropy data without EOI: either answer, but no crash
    try:
        packed = jpegdecode.entropy_decode(good[:-2])
        assert np.array_equal(R.reconstruct(packed), GOLD["g17x9_s2_rgb"])
    except ValueError:
        pass


def test_packed_size_depends_on_geometry_only():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import jpegdecode

    sizes = set()
    for k, q in enumerate((5, 50, 100)):
        data = _save(Image.fromarray(R.content(37, 29, 40 + k)), quality=q, subsampling=2, optimize=bool(k))
        packed = jpegdecode.entropy_decode(data)
        sizes.add(packed.size)
        assert packed.size == jpegdecode.packed_bytes(37, 29, 3, 2, 2)
    assert sizes == {576 + 128 * (3 * 2 * 4 + 2 * 3 * 2)}  # 3 x 2 MCUs of 4 + 1 + 1 blocks
    lib = _lib.load()
    assert lib.mr_jpeg_packed_bytes(640, 480, 3, 2, 2) == 576 + 128 * (80 * 60 + 2 * 40 * 30)
    assert lib.mr_jpeg_packed_bytes(640, 480, 3, 1, 1) == 576 + 128 * 3 * 80 * 60
    assert lib.mr_jpeg_packed_bytes(23, 11, 1, 1, 1) == 576 + 128 * 3 * 2
    assert lib.mr_jpeg_packed_bytes(1, 1, 3, 2, 1) == 576 + 128 * 4
    for bad in ((0, 8, 3, 1, 1), (8, 10753, 3, 1, 1), (8, 8, 2, 1, 1), (8, 8, 3, 1, 2), (8, 8, 3, 4, 1), (8, 8, 1, 2, 2)):
        assert lib.mr_jpeg_packed_bytes(*bad) == -1, bad
    for name in ("g17x9_s1", "grey23x11", "rst2_37x29_s2"):  # the packed frame's header repeats what jpeg_info reads
        data = GOLD[name + "_stream"].tobytes()
        assert jpegdecode.packed_info(jpegdecode.entropy_decode(data)) == jpegdecode.jpeg_info(data)
    hdr = np.frombuffer(packed[:64].tobytes(), np.int32)
    assert list(hdr[:9]) == [_lib.JPEG_MAGIC, 37, 29, 3, 2, 2, 0, 1, 1] and hdr[10] == packed.size


def test_reconstruct_argument_validation_needs_no_device():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import jpegdecode

    lib = _lib.load()
    null, p16 = ctypes.c_void_p(None), ctypes.c_void_p(0x1000)
    geom = (16, 16, 3, 2, 2)
    need = lib.mr_jpeg_reconstruct_workspace_bytes(2, *geom)
    assert need == 2 * 64 * 6
    assert lib.mr_jpeg_reconstruct_workspace_bytes(-1, *geom) == -1 and lib.mr_jpeg_reconstruct_workspace_bytes(1, 16, 16, 3, 1, 2) == -1
    assert lib.mr_jpeg_reconstruct(null, 0, *geom, null, null, 0, None) == 0  # n == 0: nothing is touched
    assert lib.mr_jpeg_reconstruct(null, 0, 16, 16, 3, 3, 1, null, null, 0, None) == -1  # ... after the geometry
    assert lib.mr_jpeg_reconstruct(p16, -1, *geom, p16, p16, need, None) == -1
    assert lib.mr_jpeg_reconstruct(null, 2, *geom, p16, p16, need, None) == -1
    assert lib.mr_jpeg_reconstruct(p16, 2, *geom, null, p16, need, None) == -1
    assert lib.mr_jpeg_reconstruct(p16, 2, *geom, p16, null, need, None) == -1
    assert lib.mr_jpeg_reconstruct(ctypes.c_void_p(0x1008), 2, *geom, p16, p16, need, None) == -1  # misaligned
    assert lib.mr_jpeg_reconstruct(p16, 2, *geom, ctypes.c_void_p(0x1002), p16, need, None) == -1
    assert lib.mr_jpeg_reconstruct(p16, 2, *geom, p16, ctypes.c_void_p(0x1008), need, None) == -1
    assert lib.mr_jpeg_reconstruct(p16, 2, *geom, p16, p16, need - 1, None) == -1  # workspace too small
    assert lib.mr_jpeg_reconstruct(p16, 2, 0, 16, 3, 2, 2, p16, p16, need, None) == -1
    assert lib.mr_jpeg_reconstruct(p16, 2, 16, 16, 4, 1, 1, p16, p16, need, None) == -1
    assert lib.mr_jpeg_reconstruct(p16, 65535, 10752, 10752, 1, 1, 1, p16, p16, 1 << 62, None) == -2  # a launch's grid
    assert lib.mr_jpeg_info(null, 0, null) == -1 and lib.mr_jpeg_entropy_decode(null, 0, null, 0) == -1
    # the Python layer checks the frames' headers on the host, before anything is uploaded
    a = jpegdecode.entropy_decode(GOLD["g16x16_s2_stream"].tobytes())
    b = jpegdecode.entropy_decode(GOLD["g16x16_s0_stream"].tobytes())
    c = jpegdecode.entropy_decode(GOLD["g8x8_s2_stream"].tobytes())  # 16 x 16 and 8 x 8 at 4:2:0: one MCU, the same size
    assert a.size == c.size != b.size
    with pytest.raises(ValueError, match="different geometries"):
        jpegdecode.reconstruct(np.stack([a, c]), "cuda")
    broken = a.copy()
    broken[0] ^= 1
    with pytest.raises(ValueError, match="no packed frame"):
        jpegdecode.reconstruct(broken[None], "cuda")
    with pytest.raises(ValueError, match="does not match"):
        jpegdecode.reconstruct(np.concatenate([a, a[:128]])[None], "cuda")
    with pytest.raises(ValueError):
        jpegdecode.reconstruct(a, "cuda")  # one frame is [1, bytes]


def _datasets(decode, color_fn="device", **kw):
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=(272, 248), seed=1, sides=("right", "left"), jpeg_quality=90)
    return ds, handobjset.HandObjSet(ds, inp_res=(64, 64), color_fn=color_fn, decode=decode, sample_nb=2, sides="right", **kw)


def test_synthpose_jpeg_mode():
    from handobjectconsist_amd.datasets import jpegdecode, synthpose

    plain = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24))
    with pytest.raises(RuntimeError):
        plain.get_image_bytes(0)
    for sub, hv in ((0, (1, 1)), (1, (2, 1)), (2, (2, 2))):
        ds = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), jpeg_quality=90, jpeg_subsampling=sub)
        assert np.array_equal(ds.frames, plain.frames)
        info = jpegdecode.jpeg_info(ds.get_image_bytes(1))
        assert (info["width"], info["height"], info["luma_h"], info["luma_v"]) == (40, 24) + hv
        assert np.array_equal(ds.get_image(1), R.pillow_decode(ds.get_image_bytes(1)))
        assert ds.get_image(1).shape == (24, 40, 3) and not np.array_equal(ds.get_image(1), plain.get_image(1))


def test_device_decode_samples_carry_the_same_draws_and_leave_the_same_rng_state():
    from handobjectconsist_amd.datasets import jpegdecode

    runs = {}
    for decode in ("host", "device"):
        ds, hs = _datasets(decode)
        random.seed(11)
        torch.manual_seed(11)
        seqs = [hs[i] for i in (0, 3)]
        runs[decode] = (seqs, random.random(), torch.rand(3), ds)
    (host, hr, ht, ds), (dev, dr, dt, _) = runs["host"], runs["device"]
    assert hr == dr and torch.equal(ht, dt)
    flips = []
    for sh, sd in zip(host, dev):
        for a, b in zip(sh, sd):
            assert "frame" in a and "frame_jpeg" not in a and "frame_jpeg" in b and "frame" not in b
            assert set(a) - {"frame"} == set(b) - {"frame_jpeg"}
            assert a["flip"] == b["flip"] and np.array_equal(a["affinetrans"], b["affinetrans"])
            assert np.array_equal(a["color_plan"], b["color_plan"]) and a["color_plan"].shape == (9,)
            for k in ("camintr", "joints3d", "handverts3d", "objverts3d"):
                assert np.array_equal(a[k], b[k]), k
            assert b["frame_jpeg"].dtype == np.uint8 and b["frame_jpeg"].shape == (jpegdecode.packed_bytes(272, 248, 3, 2, 2),)
            assert np.array_equal(R.reconstruct(b["frame_jpeg"]), a["frame"])  # the same pixels, once the GPU has rebuilt them
            flips.append(a["flip"])
    assert any(flips) and not all(flips)
    # colour off: nothing but the frame differs either
    for decode in ("host", "device"):
        _, hs = _datasets(decode, color_fn=None)
        random.seed(5)
        torch.manual_seed(5)
        runs[decode] = (hs[1], random.random(), torch.rand(1))
    assert runs["host"][1:] == runs["device"][1:]
    assert all("color_plan" not in s for s in runs["device"][0]) and all("frame_jpeg" in s for s in runs["device"][0])
    assert all(np.array_equal(a["affinetrans"], b["affinetrans"]) for a, b in zip(runs["host"][0], runs["device"][0]))


def test_device_decode_needs_a_device_colour_path_and_file_bytes():
    from handobjectconsist_amd.datasets import coloraugm, handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), jpeg_quality=90)
    with pytest.raises(ValueError, match="color_fn"):
        handobjset.HandObjSet(ds, decode="device", color_fn="reference")
    with pytest.raises(ValueError, match="color_fn"):
        handobjset.HandObjSet(ds, decode="device")  # the default colour path runs on the host
    with pytest.raises(ValueError, match="color_fn"):
        handobjset.HandObjSet(ds, decode="device", color_fn=coloraugm.make_color_fn(jitter=False))
    with pytest.raises(ValueError, match="decode"):
        handobjset.HandObjSet(ds, decode="gpu", color_fn=None)
    with pytest.raises(ValueError, match="get_image_bytes"):
        handobjset.HandObjSet(object(), decode="device", color_fn=None)
    assert handobjset.HandObjSet(ds).decode == "host"


def test_a_batch_mixing_decoded_and_packed_frames_is_refused():
    from handobjectconsist_amd.datasets import handobjset, jpegdecode

    packed = jpegdecode.entropy_decode(GOLD["g16x16_s2_stream"].tobytes())
    common = dict(affinetrans=np.eye(3)[None], flip=np.zeros(1, bool))
    a = dict(common, frame=torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    b = dict(common, frame_jpeg=torch.from_numpy(packed)[None])
    with pytest.raises(ValueError, match="frame_jpeg in 1 of 2"):
        handobjset.assemble_batch([a, b], "cuda", (8, 8))
    with pytest.raises(ValueError, match="frame_jpeg"):
        handobjset.assemble_batch([dict(a, frame_jpeg=b["frame_jpeg"])], "cuda", (8, 8))
    other = jpegdecode.entropy_decode(GOLD["g16x16_s0_stream"].tobytes())
    with pytest.raises(ValueError, match="differ in size"):
        handobjset.assemble_batch([b, dict(common, frame_jpeg=torch.from_numpy(other)[None])], "cuda", (8, 8))
    with pytest.raises(ValueError, match="must be collated"):
        handobjset.assemble_batch(dict(common, frame_jpeg=torch.from_numpy(packed)), "cuda", (8, 8))


def test_sanitizer_program_runs_clean(tmp_path):
    """tests/jpeg_entropy_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer: the three fixture streams, every
    prefix of each, and seeded single-byte mutations."""
    files = []
    for name in R.SANITIZER_STREAMS:
        path = tmp_path / (name + ".jpg")
        path.write_bytes(GOLD[name + "_stream"].tobytes())
        files.append(str(path))
    exe = str(tmp_path / "jpeg_entropy_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # the runtime inside the program: it starts whatever the loader preloads
                    "-I", os.path.join(ROOT, "handobjectconsist_amd", "csrc"), os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("prefixes") == 3
