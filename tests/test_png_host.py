"""The host side of the device PNG decode, without a GPU: what ``pngdecode.inflate`` refuses and how, the packed frame's
layout, ``HandObjSet(decode="device")``'s samples on PNG bytes against ``decode="host"``'s (same draws, same RNG streams
afterwards), and ``assemble_batch``'s and ``mr_png_unfilter``'s argument checks."""
import ctypes
import io
import random
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_ref as R

SAMPLES = R.content(5, 7, 3, 23)
LINES = R.filter_lines(SAMPLES, [4, 3, 1, 2, 0, 4, 3])
GOOD = R.write_png(LINES, 5, 7, 2)


def _save(img, **opts):
    buf = io.BytesIO()
    img.save(buf, "PNG", **opts)
    return buf.getvalue()


def test_unsupported_streams_raise_not_implemented_from_the_headers():
    from handobjectconsist_amd.datasets import pngdecode

    rgb = Image.fromarray(R.smooth(12, 9, 3, 1))
    grey16 = Image.fromarray((np.arange(12 * 9).reshape(9, 12) * 500).astype(np.uint16))
    streams = [R.palette_stream(), _save(grey16), _save(rgb.convert("1")),
               _save(rgb.convert("P", palette=Image.Palette.ADAPTIVE, colors=4), bits=2),
               _save(rgb.convert("P", palette=Image.Palette.ADAPTIVE, colors=16), bits=4)]
    assert [(data[24], data[25]) for data in streams] == [(4, 3), (16, 0), (1, 0), (2, 3), (4, 3)]  # (bit depth, colour type)
    # decided from IHDR alone: rewriting it (with its CRC) is enough, the image data never get looked at
    for depth, color, interlace in ((16, 2, 0), (16, 6, 0), (16, 4, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 2, 1), (8, 0, 1),
                                    (8, 6, 1), (8, 3, 0)):
        streams.append(R.write_png(LINES, 5, 7, color, depth=depth, interlace=interlace))
    for data in streams:
        with pytest.raises(NotImplementedError):
            pngdecode.inflate(data)
        with pytest.raises(NotImplementedError):
            pngdecode.png_info(data)
    # APNG: an acTL chunk in front of the image data
    apng = R.write_png(LINES, 5, 7, 2, before_idat=R.chunk(b"acTL", struct.pack(">II", 1, 0)))
    with pytest.raises(NotImplementedError, match="APNG"):
        pngdecode.inflate(apng)


def test_every_strict_prefix_raises_value_error():
    from handobjectconsist_amd.datasets import pngdecode

    assert np.array_equal(R.reconstruct(pngdecode.inflate(GOOD)), SAMPLES)
    for n in range(len(GOOD)):
        with pytest.raises(ValueError):
            pngdecode.inflate(GOOD[:n])
    for n in range(8 + 12 + 13):  # (shorter than signature + IHDR: png_info has nothing to read either)
        with pytest.raises(ValueError):
            pngdecode.png_info(GOOD[:n])
    assert pngdecode.png_info(GOOD[:8 + 12 + 13]) == dict(width=5, height=7, channels=3, color_type=2)


def test_malformed_streams_raise_value_error():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import pngdecode

    def refused(data, match=None):
        with pytest.raises(ValueError, match=match):
            pngdecode.inflate(data)

    refused(b"\x89PNX" + GOOD[4:], "signature")
    refused(b"\xff\xd8\xff\xe0" + GOOD[4:], "signature")
    for ctype in (b"IHDR", b"IDAT", b"IEND"):  # a flipped CRC bit on each critical chunk
        at = GOOD.index(ctype)
        length, = struct.unpack_from(">I", GOOD, at - 4)
        bad = bytearray(GOOD)
        bad[at + 4 + length + 3] ^= 1
        refused(bytes(bad), "CRC")
    bad = bytearray(GOOD)  # ... and a flipped payload bit
    bad[GOOD.index(b"IDAT") + 6] ^= 0x10
    refused(bytes(bad), "CRC")
    anc = R.write_png(LINES, 5, 7, 2, before_idat=R.chunk(b"tEXt", b"k\x00v")[:-1] + b"\x00")  # an ancillary chunk's CRC is not looked at
    assert np.array_equal(pngdecode.inflate(anc), pngdecode.inflate(GOOD))
    refused(R.write_png([bytes([5]) + LINES[0][1:]] + LINES[1:], 5, 7, 2), "filter byte")
    refused(R.write_png(LINES[:3] + [bytes([255]) + LINES[3][1:]] + LINES[4:], 5, 7, 2), "filter byte")
    refused(R.write_png(LINES[:-1], 5, 7, 2), "do not inflate")          # one row short
    refused(R.write_png(LINES + LINES[:1], 5, 7, 2), "do not inflate")   # one row long
    refused(R.write_png(LINES, 5, 7, 6), "do not inflate")               # the rows of another colour type
    ihdr = struct.pack(">IIBBBBB", 5, 7, 8, 2, 0, 0, 0)
    head, idat, iend = R.SIGNATURE + R.chunk(b"IHDR", ihdr), R.chunk(b"IDAT", zlib.compress(b"".join(LINES))), R.chunk(b"IEND", b"")
    assert head + idat + iend == GOOD
    refused(R.SIGNATURE + idat + iend, "IHDR")
    refused(head + iend, "IDAT")
    refused(head + idat, "IEND")
    refused(head + head[8:] + idat + iend, "second IHDR")
    refused(head + R.chunk(b"IDAT", zlib.compress(b"".join(LINES))[:-5]) + iend)            # the zlib stream stops early
    refused(head + R.chunk(b"IDAT", b"\x78\x9c\xff\xff\xff\xff") + iend, "inflate error")
    refused(head + R.chunk(b"ABCD", b"") + idat + iend, "critical")
    refused(GOOD[:12 + 8] + struct.pack(">I", 0x7FFFFFF0) + GOOD[12 + 12:], None)           # (the CRC goes first)
    for w, h in ((0, 7), (5, 0)):
        refused(R.write_png(LINES, w, h, 2), "zero")
    for w, h in ((_lib.PNG_MAX_SIDE + 1, 7), (5, _lib.PNG_MAX_SIDE + 1)):
        refused(R.write_png(LINES, w, h, 2), "limit")
    for ihdr_bad in (dict(depth=3), dict(depth=8, color=5), dict(depth=4, color=2), dict(interlace=2)):
        kw = dict(dict(depth=8, color=2, interlace=0), **ihdr_bad)
        refused(R.write_png(LINES, 5, 7, kw["color"], depth=kw["depth"], interlace=kw["interlace"]), "invalid IHDR")
    bad = bytearray(head)
    bad[8 + 8 + 10] = 1  # compression method 1
    bad[8 + 8 + 13:8 + 8 + 17] = struct.pack(">I", zlib.crc32(bytes(bad[12:8 + 8 + 13])))
    refused(bytes(bad) + idat + iend, "invalid IHDR")
    # a chunk whose length runs past the end of the data
    bad = bytearray(GOOD)
    at = GOOD.index(b"IDAT") - 4
    bad[at:at + 4] = struct.pack(">I", len(GOOD))
    refused(bytes(bad), "past the end")


def test_idat_in_one_byte_chunks_and_data_behind_iend():
    from handobjectconsist_amd.datasets import pngdecode

    split = R.write_png(LINES, 5, 7, 2, idat_bytes=1)
    assert split.count(b"IDAT") == len(zlib.compress(b"".join(LINES)))
    assert np.array_equal(pngdecode.inflate(split), pngdecode.inflate(GOOD))
    assert np.array_equal(R.pillow_decode(split), SAMPLES)
    assert np.array_equal(pngdecode.inflate(GOOD + b"trailing"), pngdecode.inflate(GOOD))
    assert np.array_equal(pngdecode.inflate(np.frombuffer(GOOD, np.uint8)), pngdecode.inflate(GOOD))


def test_packed_frame_layout_depends_on_geometry_only():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import pngdecode

    packed = pngdecode.inflate(GOOD)
    assert packed.dtype == np.uint8 and packed.size == pngdecode.packed_bytes(5, 7, 3) == (64 + 7 * 16 + 15) // 16 * 16
    hdr = np.frombuffer(packed[:64].tobytes(), np.int32)
    assert list(hdr[:5]) == [_lib.PNG_MAGIC, 5, 7, 3, 2] and not hdr[5:].any()
    assert packed[64:64 + 7 * 16].tobytes() == b"".join(LINES) and not packed[64 + 7 * 16:].any()
    sizes = {pngdecode.inflate(R.pillow_encode(R.smooth(37, 29, 3, k), dict(compress_level=k))).size for k in (0, 3, 9)}
    assert sizes == {pngdecode.packed_bytes(37, 29, 3)}
    lib = _lib.load()
    assert (R.MAGIC, R.HEADER_BYTES, R.BAND_ROWS) == (_lib.PNG_MAGIC, _lib.PNG_HEADER_BYTES, _lib.PNG_BAND_ROWS)
    for w, h, c in ((5, 7, 3), (640, 480, 3), (1, 1, 1), (67, 6, 4), (_lib.PNG_MAX_SIDE, 3, 2)):
        assert lib.mr_png_packed_bytes(w, h, c) == pngdecode.packed_bytes(w, h, c) == (64 + h * (1 + w * c) + 15) // 16 * 16
        assert lib.mr_png_unfilter_workspace_bytes(3, w, h, c) == 0
    for bad in ((0, 7, 3), (5, 0, 3), (5, 7, 0), (5, 7, 5), (_lib.PNG_MAX_SIDE + 1, 7, 3), (5, _lib.PNG_MAX_SIDE + 1, 3)):
        assert lib.mr_png_packed_bytes(*bad) == -1 and lib.mr_png_unfilter_workspace_bytes(1, *bad) == -1, bad
        with pytest.raises(ValueError):
            pngdecode.packed_bytes(*bad)
    assert lib.mr_png_unfilter_workspace_bytes(-1, 5, 7, 3) == -1


def test_the_header_states_the_constants_of_the_binding():
    import os
    import re

    from handobjectconsist_amd import _lib

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "meshraster_hip.h")).read()
    for name, value in (("MAGIC", _lib.PNG_MAGIC), ("HEADER_BYTES", _lib.PNG_HEADER_BYTES), ("BAND_ROWS", _lib.PNG_BAND_ROWS),
                        ("MAX_SIDE", _lib.PNG_MAX_SIDE)):
        assert int(re.search(r"#define MR_PNG_" + name + r"\s+(\S+)", src).group(1), 0) == value, name
    assert _lib.ABI_VERSION == 9  # additions only


def test_unfilter_argument_validation_needs_no_device():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import pngdecode

    lib = _lib.load()
    null, p16 = ctypes.c_void_p(None), ctypes.c_void_p(0x1000)
    assert lib.mr_png_unfilter(null, 0, 5, 7, 3, null, null, None) == 0  # n == 0: nothing is touched
    assert lib.mr_png_unfilter(null, 0, 5, 7, 5, null, null, None) == -1  # ... after the geometry
    assert lib.mr_png_unfilter(p16, -1, 5, 7, 3, p16, null, None) == -1
    assert lib.mr_png_unfilter(null, 2, 5, 7, 3, p16, null, None) == -1
    assert lib.mr_png_unfilter(p16, 2, 5, 7, 3, null, null, None) == -1
    assert lib.mr_png_unfilter(ctypes.c_void_p(0x1008), 2, 5, 7, 3, p16, null, None) == -1  # misaligned
    assert lib.mr_png_unfilter(p16, 2, 5, 7, 3, ctypes.c_void_p(0x1002), null, None) == -1
    for w, h, c in ((0, 7, 3), (5, -1, 3), (5, 7, 0), (5, 7, 5)):
        assert lib.mr_png_unfilter(p16, 2, w, h, c, p16, null, None) == -1
    assert lib.mr_png_unfilter(p16, 2, _lib.PNG_MAX_SIDE + 1, 7, 3, p16, null, None) == -2
    assert lib.mr_png_unfilter(p16, 2, 5, _lib.PNG_MAX_SIDE + 1, 3, p16, null, None) == -2
    # the Python layer checks the frames' headers and filter bytes on the host, before anything is uploaded
    a = pngdecode.inflate(GOOD)
    b = pngdecode.inflate(R.write_png(R.filter_lines(R.content(5, 7, 4, 1), [0] * 7), 5, 7, 6))
    c = pngdecode.inflate(R.write_png(R.filter_lines(R.content(7, 5, 3, 1), [0] * 5), 7, 5, 2))  # 7 x 16 and 5 x 22 bytes: one size
    d = pngdecode.inflate(R.write_png(R.filter_lines(R.content(10, 7, 3, 1), [0] * 7), 10, 7, 2))
    assert a.size == c.size and a.size != b.size and a.size != d.size
    with pytest.raises(ValueError, match="different geometries"):
        pngdecode.unfilter(np.stack([a, c]), "cuda")
    broken = a.copy()
    broken[0] ^= 1
    with pytest.raises(ValueError, match="no packed frame"):
        pngdecode.unfilter(broken[None], "cuda")
    with pytest.raises(ValueError, match="does not match"):
        pngdecode.unfilter(np.concatenate([a, a[:16]])[None], "cuda")
    with pytest.raises(ValueError):
        pngdecode.unfilter(a, "cuda")  # one frame is [1, bytes]
    with pytest.raises(ValueError, match="empty"):
        pngdecode.unfilter(np.zeros((0, a.size), np.uint8), "cuda")
    five = a.copy()
    five[64 + 3 * 16] = 5
    with pytest.raises(ValueError, match="filter byte"):
        pngdecode.unfilter(np.stack([a, five]), "cuda")
    with pytest.raises(ValueError, match="unsupported"):
        pngdecode.decode_batch([GOOD], "cuda", unsupported="skip")
    with pytest.raises(ValueError, match="at least one"):
        pngdecode.decode_batch([], "cuda")
    with pytest.raises(NotImplementedError):
        pngdecode.decode_batch([GOOD, R.palette_stream()], "cuda")


def _datasets(decode, color_fn="device", **kw):
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=(92, 70), seed=1, sides=("right", "left"), png_compress_level=1)
    return ds, handobjset.HandObjSet(ds, inp_res=(64, 64), color_fn=color_fn, decode=decode, sample_nb=2, sides="right", **kw)


def test_synthpose_png_mode():
    from handobjectconsist_amd.datasets import pngdecode, synthpose

    plain = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24))
    with pytest.raises(RuntimeError):
        plain.get_image_bytes(0)
    with pytest.raises(ValueError, match="one format"):
        synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), jpeg_quality=90, png_compress_level=6)
    sizes = []
    for level in (0, 6):
        ds = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), png_compress_level=level)
        assert np.array_equal(ds.frames, plain.frames)
        data = ds.get_image_bytes(1)
        assert data[:8] == pngdecode.SIGNATURE
        assert pngdecode.png_info(data) == dict(width=40, height=24, channels=3, color_type=2)
        assert np.array_equal(ds.get_image(1), R.pillow_decode(data)) and np.array_equal(ds.get_image(1), plain.get_image(1))
        sizes.append(len(data))
    assert sizes[0] > sizes[1] or sizes[0] > 40 * 24 * 3  # (level 0 stores)
    jpeg = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), jpeg_quality=90)  # ... and the JPEG mode is as it was
    assert jpeg.get_image_bytes(0)[:2] == b"\xff\xd8"


def test_device_decode_samples_carry_the_same_draws_and_leave_the_same_rng_state():
    from handobjectconsist_amd.datasets import pngdecode

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
            assert "frame" in a and "frame_png" not in a and "frame_png" in b and "frame" not in b and "frame_jpeg" not in b
            assert set(a) - {"frame"} == set(b) - {"frame_png"}
            assert a["flip"] == b["flip"] and np.array_equal(a["affinetrans"], b["affinetrans"])
            assert np.array_equal(a["color_plan"], b["color_plan"]) and a["color_plan"].shape == (9,)
            for k in ("camintr", "joints3d", "handverts3d", "objverts3d"):
                assert np.array_equal(a[k], b[k]), k
            assert b["frame_png"].dtype == np.uint8 and b["frame_png"].shape == (pngdecode.packed_bytes(92, 70, 3),)
            assert np.array_equal(R.reconstruct(b["frame_png"]), a["frame"])  # the same pixels, once the GPU has rebuilt them
            flips.append(a["flip"])
    assert any(flips) and not all(flips)
    # colour off: nothing but the frame differs either
    for decode in ("host", "device"):
        _, hs = _datasets(decode, color_fn=None)
        random.seed(5)
        torch.manual_seed(5)
        runs[decode] = (hs[1], random.random(), torch.rand(1))
    assert runs["host"][1:] == runs["device"][1:]
    assert all("color_plan" not in s for s in runs["device"][0]) and all("frame_png" in s for s in runs["device"][0])
    assert all(np.array_equal(a["affinetrans"], b["affinetrans"]) for a, b in zip(runs["host"][0], runs["device"][0]))


def test_device_decode_keeps_its_constraints_and_sends_other_bytes_the_jpeg_way():
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), png_compress_level=6)
    with pytest.raises(ValueError, match="color_fn"):
        handobjset.HandObjSet(ds, decode="device", color_fn="reference")
    with pytest.raises(ValueError, match="color_fn"):
        handobjset.HandObjSet(ds, decode="device")
    assert handobjset.HandObjSet(ds).decode == "host"
    jpeg = synthpose.SynthPoseDataset(num_pairs=1, frame_size=(40, 24), jpeg_quality=90)
    sample = handobjset.HandObjSet(jpeg, inp_res=(16, 16), color_fn=None, decode="device")[0]
    assert "frame_jpeg" in sample and "frame_png" not in sample

    class Garbage:
        def __getattr__(self, name):
            return getattr(ds, name)

        def get_image_bytes(self, idx):
            return b"\x89PNG\r\n\x1a" + b"?" * 40  # seven bytes of the signature: not PNG, so the JPEG stage's error

    with pytest.raises(ValueError, match="JPEG"):
        handobjset.HandObjSet(Garbage(), inp_res=(16, 16), color_fn=None, decode="device").get_sample(0)


def test_a_batch_mixing_frame_kinds_is_refused():
    from handobjectconsist_amd.datasets import handobjset, jpegdecode, pngdecode

    packed = pngdecode.inflate(GOOD)
    common = dict(affinetrans=np.eye(3)[None], flip=np.zeros(1, bool))
    a = dict(common, frame=torch.zeros(1, 7, 5, 3, dtype=torch.uint8))
    b = dict(common, frame_png=torch.from_numpy(packed)[None])
    buf = io.BytesIO()
    Image.fromarray(R.smooth(16, 16, 3, 2)).save(buf, "JPEG", quality=90)
    c = dict(common, frame_jpeg=torch.from_numpy(jpegdecode.entropy_decode(buf.getvalue()))[None])
    with pytest.raises(ValueError, match="frame_png in 1 of 2"):
        handobjset.assemble_batch([a, b], "cuda", (8, 8))
    with pytest.raises(ValueError, match="in 1 of 2"):
        handobjset.assemble_batch([c, b], "cuda", (8, 8))
    with pytest.raises(ValueError, match="frame_png"):
        handobjset.assemble_batch([dict(a, frame_png=b["frame_png"])], "cuda", (8, 8))
    with pytest.raises(ValueError, match="frame_jpeg"):
        handobjset.assemble_batch([dict(c, frame_png=b["frame_png"])], "cuda", (8, 8))
    other = pngdecode.inflate(R.write_png(R.filter_lines(R.content(10, 7, 3, 1), [0] * 7), 10, 7, 2))
    with pytest.raises(ValueError, match="differ in size"):
        handobjset.assemble_batch([b, dict(common, frame_png=torch.from_numpy(other)[None])], "cuda", (8, 8))
    with pytest.raises(ValueError, match="must be collated"):
        handobjset.assemble_batch(dict(common, frame_png=torch.from_numpy(packed)), "cuda", (8, 8))
