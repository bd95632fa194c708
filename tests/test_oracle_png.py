"""The host stage of the PNG decode (``pngdecode.inflate``) followed by the restatement of the unfilter (tests/png_ref.py)
against the INSTALLED Pillow, every byte: pins both on a box without a GPU, before any kernel is involved.  The cases are
built live; tests/golden/png_pil.npz records the same ones."""
import io
import json
import os
import struct

import numpy as np
import pytest
from PIL import Image

from tests import png_ref as R

STREAMS = R.all_streams()
HAND = R.hand_cases()


@pytest.mark.parametrize("name", list(STREAMS))
def test_inflate_plus_restatement_equals_pillow(name):
    from handobjectconsist_amd.datasets import pngdecode

    data = STREAMS[name]
    want = R.pillow_decode(data)
    packed = pngdecode.inflate(data)
    got = R.reconstruct(packed)
    assert got.shape == want.shape and int((got != want).sum()) == 0
    img = Image.open(io.BytesIO(data))
    info = pngdecode.png_info(data)
    assert (info["width"], info["height"]) == img.size and R.MODES[info["channels"]] == img.mode
    assert pngdecode.packed_info(packed) == info and packed.size == pngdecode.packed_bytes(*img.size, info["channels"])
    if name in HAND:  # Pillow reads the hand-made streams as the samples they were made from
        samples, filters = HAND[name]
        assert np.array_equal(want, R.to_rgb(samples))
        stride = 1 + samples.shape[1] * samples.shape[2]
        assert list(packed[R.HEADER_BYTES:R.HEADER_BYTES + samples.shape[0] * stride:stride]) == list(filters)


def test_the_cases_cover_what_they_claim():
    """Paeth ties of all three kinds, averages that pass 255, all five filters in Pillow's own streams taken together, IDAT
    split differently by the compression levels."""
    for name in ("paeth_ties_c1", "paeth_ties_c3"):
        s = HAND[name][0].astype(int)
        a, b, c = s[1:, :-1], s[:-1, 1:], s[:-1, :-1]
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        assert ((pa == pb) & (pa < pc)).any() and ((pb == pc) & (pb < pa)).any() and ((pa == pb) & (pb == pc)).any()
        assert ((pa == pc) & (pa < pb)).any()
    s = R.AVERAGE_CARRY.astype(int)
    assert (s[1:, :-1] + s[:-1, 1:] >= 256).all()
    from handobjectconsist_amd.datasets import pngdecode

    used = set()
    for name in R.pillow_cases():
        packed = pngdecode.inflate(STREAMS[name])
        h = R.parse_header(packed)
        stride = 1 + h["width"] * h["channels"]
        used |= set(int(v) for v in packed[R.HEADER_BYTES:R.HEADER_BYTES + h["height"] * stride:stride])
    assert used >= {1, 2, 4}, used  # (what Pillow's adaptive choice takes on these frames; the hand-made streams force all five)
    sizes = {len(STREAMS[f"pil_level{k}"]) for k in (0, 1, 9)}
    assert len(sizes) == 3


def test_idat_split_and_ancillary_chunks_do_not_matter():
    from handobjectconsist_amd.datasets import pngdecode

    samples, filters = HAND["f43120_5x7_c3"]
    lines = R.filter_lines(samples, filters)
    whole = pngdecode.inflate(R.write_png(lines, 5, 7, 2))
    for step in (1, 2, 7):
        data = R.write_png(lines, 5, 7, 2, idat_bytes=step)
        assert data.count(b"IDAT") > 3 and np.array_equal(pngdecode.inflate(data), whole)
        assert np.array_equal(R.pillow_decode(data), R.to_rgb(samples))
    extra = R.chunk(b"tEXt", b"Comment\x00hello") + R.chunk(b"gAMA", struct.pack(">I", 45455)) + R.chunk(b"pHYs", b"\0" * 9)
    data = R.write_png(lines, 5, 7, 2, before_idat=extra)
    assert np.array_equal(pngdecode.inflate(data), whole) and np.array_equal(R.pillow_decode(data), R.to_rgb(samples))


@pytest.mark.parametrize("channels", [1, 3])
def test_a_trns_chunk_is_ignored_as_pillow_ignores_it(channels):
    """tRNS on colour types 0 and 2 names one transparent colour; ``convert("RGB")`` of the installed Pillow gives the plain
    samples all the same, so the host stage skips the chunk like every ancillary one."""
    from handobjectconsist_amd.datasets import pngdecode

    samples = R.content(6, 5, channels, 7, 0, 3)  # few values: the transparent colour occurs
    colour = [int(v) for v in samples[2, 3]]
    trns = R.chunk(b"tRNS", b"".join(struct.pack(">H", v) for v in colour))
    data = R.write_png(R.filter_lines(samples, R.cycle(5)), 6, 5, R.COLOR_OF[channels], before_idat=trns)
    img = Image.open(io.BytesIO(data))
    assert "transparency" in img.info
    want = np.asarray(img.convert("RGB"))
    assert np.array_equal(want, R.to_rgb(samples))
    assert np.array_equal(R.reconstruct(pngdecode.inflate(data)), want)


def test_the_fixture_records_the_same_streams_and_pixels():
    """tests/golden/png_pil.npz against the installed Pillow: decoding the RECORDED streams gives the recorded pixels, and
    the hand-made streams (no encoder of Pillow's involved) hold the scanlines the case list builds today."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "png_pil.npz"))
    names = json.loads(str(gold["meta"]))["names"]
    assert names == list(STREAMS)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "png_pil.npz")) < 200 * 1024
    for name in names + ["palette"]:
        assert np.array_equal(R.pillow_decode(gold[name + "_stream"].tobytes()), gold[name + "_rgb"]), name
    from handobjectconsist_amd.datasets import pngdecode

    for name in HAND:  # (the scanlines, not the streams: another zlib build may compress them differently)
        assert np.array_equal(pngdecode.inflate(gold[name + "_stream"].tobytes()), pngdecode.inflate(STREAMS[name])), name
