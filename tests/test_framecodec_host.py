"""``datasets/framecodec.py`` without a GPU: which codec a file's bytes get, that each codec's record is its module's own
functions, that the shared driver refuses what both modules' ``decode_batch`` refuse, and that the shared code exists once."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_ref, png_ref


def _jpeg_stream(**opts):
    buf = io.BytesIO()
    Image.fromarray(jpeg_ref.content(16, 16, 3)).save(buf, "JPEG", quality=90, **opts)
    return buf.getvalue()


JPEG = _jpeg_stream()
PNG = png_ref.pillow_encode(png_ref.smooth(16, 16, 3, 4), {})
# per codec key: (a stream, the module's host stage, the numpy restatement of the device stage, a stream the host stage refuses)
CASES = {"frame_jpeg": (JPEG, "entropy_decode", jpeg_ref.reconstruct, _jpeg_stream(progressive=True)),
         "frame_png": (PNG, "inflate", png_ref.reconstruct, png_ref.palette_stream())}


def _module(key):
    from handobjectconsist_amd.datasets import jpegdecode, pngdecode

    return {"frame_jpeg": jpegdecode, "frame_png": pngdecode}[key]


def test_codec_for_goes_by_the_whole_png_signature():
    from handobjectconsist_amd.datasets import framecodec, jpegdecode, pngdecode

    assert {c.key for c in framecodec.CODECS} == {"frame_jpeg", "frame_png"} and len(framecodec.CODECS) == 2
    assert framecodec.codec_for(PNG) is pngdecode.CODEC and pngdecode.CODEC.key == "frame_png"
    assert framecodec.codec_for(np.frombuffer(PNG, np.uint8)) is pngdecode.CODEC
    assert framecodec.codec_for(JPEG) is jpegdecode.CODEC and jpegdecode.CODEC.key == "frame_jpeg"
    garbage = b"\x89PNG\r\n\x1a" + b"?" * 40  # seven bytes of the signature: the JPEG way, whose error then names JPEG
    codec = framecodec.codec_for(garbage)
    assert codec is jpegdecode.CODEC
    with pytest.raises(ValueError, match="JPEG"):
        codec.host_stage(garbage)
    assert framecodec.codec_for(b"") is jpegdecode.CODEC


@pytest.mark.parametrize("key", sorted(CASES))
def test_a_codec_is_its_modules_own_stages(key):
    from handobjectconsist_amd.datasets import framecodec

    data, host_stage, restated, _ = CASES[key]
    codec = {c.key: c for c in framecodec.CODECS}[key]
    assert codec is framecodec.codec_for(data) is _module(key).CODEC
    packed = codec.host_stage(data)
    own = getattr(_module(key), host_stage)(data)
    assert packed.dtype == np.uint8 and packed.ndim == 1 and packed.tobytes() == own.tobytes()
    info = codec.packed_info(packed)
    assert (info["width"], info["height"]) == (16, 16)
    assert codec.batch_geometry(np.stack([packed, packed]))[:2] == (16, 16)
    assert codec.geometry_header_bytes <= packed.size and codec.geometry_header_bytes == {"frame_jpeg": 24, "frame_png": 16}[key]
    want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert want.shape == (16, 16, 3) and np.array_equal(restated(packed), want)
    fallback = framecodec.pillow_rgb(data)
    assert np.array_equal(fallback, want) and fallback.flags.writeable


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_shared_driver_refuses_what_the_modules_refuse(key):
    from handobjectconsist_amd.datasets import framecodec

    data, _, _, refused = CASES[key]
    codec = _module(key).CODEC
    for decode_batch in (lambda *a, **k: framecodec.decode_batch(codec, *a, **k), _module(key).decode_batch):
        with pytest.raises(ValueError, match="unsupported"):
            decode_batch([data], "cuda", unsupported="skip")
        with pytest.raises(ValueError, match="unsupported"):
            decode_batch([], "cuda", unsupported="skip")  # (checked first)
        with pytest.raises(ValueError, match="at least one"):
            decode_batch([], "cuda")
        for threads in (None, 1):
            with pytest.raises(NotImplementedError):
                decode_batch([data, refused], "cuda", threads=threads)
            with pytest.raises(NotImplementedError):
                decode_batch([data, refused], "cuda", threads=threads, unsupported="raise")
    for decode_packed in (lambda *a: framecodec.decode_packed(codec, *a), getattr(_module(key), {"frame_jpeg": "reconstruct", "frame_png": "unfilter"}[key])):
        packed = codec.host_stage(data)
        with pytest.raises(ValueError, match="empty"):
            decode_packed(np.zeros((0, packed.size), np.uint8), "cuda")
        broken = packed.copy()
        broken[0] ^= 1
        with pytest.raises(ValueError, match="no packed frame"):
            decode_packed(broken[None], "cuda")


def test_the_shared_code_exists_once():
    from handobjectconsist_amd.datasets import framecodec, jpegdecode, pngdecode

    for module in (jpegdecode, pngdecode):
        for name in ("_as_bytes", "_pillow_rgb", "ThreadPoolExecutor", "concurrent", "io"):
            assert not hasattr(module, name), (module.__name__, name)
        assert module.framecodec is framecodec
    for name in ("as_bytes", "pillow_rgb", "ThreadPoolExecutor", "decode_packed", "decode_batch", "codec_for", "Codec"):
        assert hasattr(framecodec, name), name
    assert framecodec.as_bytes(np.frombuffer(PNG, np.uint8)) == PNG == framecodec.as_bytes(bytearray(PNG))
