"""The host stage of the JPEG decode (``jpegdecode.entropy_decode`` through the built library) followed by the numpy
restatement of the reconstruction (tests/jpeg_ref.py) against the INSTALLED Pillow, every byte: pins both on a box without
a GPU, before any kernel is involved.  The cases are encoded live; tests/golden/jpeg_pil.npz records the same ones."""
import io
import json
import os

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_ref as R

CASES = R.case_list()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_entropy_decode_plus_restatement_equals_pillow(case):
    from handobjectconsist_amd.datasets import jpegdecode

    data = R.encode(case)
    want = R.pillow_decode(data)
    assert want.shape == (case[2], case[1], 3)
    got = R.reconstruct(jpegdecode.entropy_decode(data))
    assert got.shape == want.shape and int((got != want).sum()) == 0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_jpeg_info_agrees_with_pillow(case):
    from handobjectconsist_amd.datasets import jpegdecode

    data = R.encode(case)
    img = Image.open(io.BytesIO(data))
    info = jpegdecode.jpeg_info(data)
    assert (info["width"], info["height"]) == img.size
    assert info["components"] == len(img.layer) == (1 if case[3] == "L" else 3)
    if info["components"] == 3:
        assert (info["luma_h"], info["luma_v"]) == tuple(img.layer[0][1:3])
        assert all(tuple(layer[1:3]) == (1, 1) for layer in img.layer[1:])
    assert info["restart_interval"] == case[5].get("restart_marker_blocks", 0)


def test_the_cases_cover_what_they_claim():
    """Stuffed 0xFF bytes at quality 100, restart markers where asked for, custom Huffman tables with optimize, DC-only
    blocks at quality 5, quantisers of 1 at quality 100."""
    from handobjectconsist_amd.datasets import jpegdecode

    by_name = {c[0]: c for c in CASES}
    assert b"\xff\x00" in R.encode(by_name["q100_37x29_s0"])
    rst = R.encode(by_name["rst1_37x29_s2"])  # 6 MCUs: RST0..4
    assert all(bytes([0xFF, 0xD0 + k]) in rst for k in range(5))
    rst = R.encode(by_name["rst1_48x40_s0"])  # 30 MCUs: the numbers wrap
    assert all(rst.count(bytes([0xFF, 0xD0 + k])) >= 3 for k in range(8))
    assert len(R.encode(by_name["optimize_37x29_s2"])) < len(R.encode(by_name["g37x29_s2"]))
    q5 = jpegdecode.entropy_decode(R.encode(by_name["q5_37x29_s2"]))
    coef = np.frombuffer(q5[R.HEADER_BYTES:].tobytes(), np.int16).reshape(-1, 64)
    assert (np.abs(coef[:, 1:]).sum(1) == 0).sum() >= 8  # DC-only blocks
    assert np.frombuffer(q5[64:R.HEADER_BYTES].tobytes(), np.uint16).max() == 255  # the largest 8-bit quantiser
    q100 = jpegdecode.entropy_decode(R.encode(by_name["q100_37x29_s0"]))
    quant = np.frombuffer(q100[64:R.HEADER_BYTES].tobytes(), np.uint16).reshape(4, 64)
    assert (quant[:2] == 1).all()


def test_the_fixture_records_the_same_streams_and_pixels():
    """tests/golden/jpeg_pil.npz against the installed Pillow: decoding the RECORDED streams gives the recorded pixels."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "jpeg_pil.npz"))
    names = json.loads(str(gold["meta"]))["names"]
    assert names == [c[0] for c in CASES]
    for name in names + ["progressive"]:
        assert np.array_equal(R.pillow_decode(gold[name + "_stream"].tobytes()), gold[name + "_rgb"]), name
