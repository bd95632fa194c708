"""PNG files -> decoded frames in two stages: the serial half of a decode -- chunk parsing and zlib
inflate -- on the host (``inflate``: bytes -> one PACKED FRAME, a flat uint8 array whose size depends on the geometry only:
a 64-byte header, then the filtered scanlines exactly as inflated), the parallel half -- undoing the per-row prediction
filters, dropping alpha / replicating grey -- on the GPU (``unfilter``: a stacked batch of packed frames -> uint8 CUDA
[N,H,W,3], byte for byte what Pillow's ``Image.open(...).convert("RGB")`` gives; the tensor ``frames.color_augment`` /
``frames.frames_to_batch`` take).

8-bit, non-interlaced streams of colour type 0 (grey), 2 (RGB), 4 (grey + alpha) and 6 (RGBA), any number of IDAT chunks;
ancillary chunks are skipped -- tRNS among them: ``convert("RGB")`` ignores it for these colour types
(tests/test_oracle_png.py holds that against the installed Pillow).  Palette, other bit depths, Adam7 and APNG raise
NotImplementedError from the headers alone -- ``decode_batch`` can hand exactly those files to Pillow on request, never
silently; malformed streams raise ValueError.  Plain Python and the standard library's zlib, which releases the GIL."""
import struct
import zlib

import numpy as np

from handobjectconsist_amd import _lib
from handobjectconsist_amd.datasets import framecodec

SIGNATURE = b"\x89PNG\r\n\x1a\n"
INFO_FIELDS = ("width", "height", "channels", "color_type")
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}  # colour type -> bytes per pixel at bit depth 8
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}  # the specification's combinations
_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")


def _chunk(data, pos):
    """(type, payload start, payload end, position of the next chunk) of the chunk at ``pos``; critical chunks' CRCs checked."""
    if pos + 8 > len(data):
        raise ValueError("PNG: truncated (a chunk header runs past the end of the data)")
    length, = struct.unpack_from(">I", data, pos)
    ctype = data[pos + 4:pos + 8]
    end = pos + 8 + length
    if length > 0x7FFFFFFF or end + 4 > len(data):
        raise ValueError(f"PNG: truncated (chunk {ctype!r} runs past the end of the data)")
    if ctype in _CRITICAL and zlib.crc32(data[pos + 4:end]) != struct.unpack_from(">I", data, end)[0]:
        raise ValueError(f"PNG: CRC mismatch in chunk {ctype!r}")
    return ctype, pos + 8, end, end + 4


def _header(data):
    """Signature + IHDR -> (width, height, channels, colour type, position of the chunk after IHDR)."""
    if data[:8] != SIGNATURE:
        raise ValueError("PNG: bad signature")
    ctype, lo, hi, pos = _chunk(data, 8)
    if ctype != b"IHDR" or hi - lo != 13:
        raise ValueError("PNG: the first chunk is no IHDR")
    width, height, depth, color, compression, filt, interlace = struct.unpack_from(">IIBBBBB", data, lo)
    if color not in _DEPTHS or depth not in _DEPTHS[color] or compression != 0 or filt != 0 or interlace > 1:
        raise ValueError("PNG: invalid IHDR")
    if width == 0 or height == 0:
        raise ValueError("PNG: a frame side is zero")
    if color == 3 or depth != 8 or interlace:
        raise NotImplementedError("PNG: only 8-bit, non-interlaced grey / RGB streams with or without alpha are decoded here "
                                  f"(colour type {color}, bit depth {depth}, interlace {interlace})")
    if width > _lib.PNG_MAX_SIDE or height > _lib.PNG_MAX_SIDE:
        raise ValueError(f"PNG: {width} x {height} is beyond the device stage's limit of {_lib.PNG_MAX_SIDE} pixels a side")
    return width, height, CHANNELS[color], color, pos


def png_info(data):
    """Geometry of a PNG stream from its signature and IHDR: dict of ``INFO_FIELDS``.  ValueError for malformed headers,
    NotImplementedError for streams ``inflate`` does not support."""
    return dict(zip(INFO_FIELDS, _header(framecodec.as_bytes(data))[:4]))


def packed_bytes(width, height, channels):
    """Bytes of a packed frame: the header, ``height`` scanlines of ``1 + width * channels`` bytes, padded to 16."""
    if not (1 <= width <= _lib.PNG_MAX_SIDE and 1 <= height <= _lib.PNG_MAX_SIDE and 1 <= channels <= 4):
        raise ValueError("not a supported frame geometry")
    return (_lib.PNG_HEADER_BYTES + height * (1 + width * channels) + 15) & ~15


def inflate(data):
    """bytes of one PNG file -> its packed frame, np.uint8 [packed_bytes(geometry)] (the layout: include/meshraster_hip.h).
    Needs no device and no compiled code."""
    data = framecodec.as_bytes(data)
    width, height, channels, color, pos = _header(data)
    idat, ended = [], False
    while pos < len(data):
        ctype, lo, hi, pos = _chunk(data, pos)
        if ctype == b"IEND":
            ended = True
            break
        if ctype == b"IDAT":
            idat.append(data[lo:hi])
        elif ctype == b"IHDR":
            raise ValueError("PNG: a second IHDR")
        elif ctype in (b"acTL", b"fcTL", b"fdAT"):
            raise NotImplementedError("PNG: animated streams (APNG) are not decoded here")
        elif not ctype[0] & 0x20 and ctype != b"PLTE":
            raise ValueError(f"PNG: unknown critical chunk {ctype!r}")
    if not idat:
        raise ValueError("PNG: no IDAT chunk")
    if not ended:
        raise ValueError("PNG: no IEND chunk")
    stride = 1 + width * channels
    want = height * stride
    unz = zlib.decompressobj()
    try:
        raw = unz.decompress(b"".join(idat), want + 1)
    except zlib.error as e:
        raise ValueError(f"PNG: inflate error ({e})") from None
    if len(raw) != want or not unz.eof:
        raise ValueError(f"PNG: the image data do not inflate to height * (1 + width * channels) = {want} bytes")
    packed = np.zeros(packed_bytes(width, height, channels), np.uint8)
    packed[:20].view(np.int32)[:] = (_lib.PNG_MAGIC, width, height, channels, color)
    body = packed[_lib.PNG_HEADER_BYTES:_lib.PNG_HEADER_BYTES + want]
    body[:] = np.frombuffer(raw, np.uint8)
    if int(body[::stride].max()) > 4:  # all H filter bytes, one strided view: the device stage never sees an unknown filter
        raise ValueError("PNG: a scanline's filter byte is above 4")
    return packed


def packed_info(packed):
    """The geometry a packed frame carries in its header: dict of ``INFO_FIELDS`` (no parse of the file)."""
    hdr = np.ascontiguousarray(packed[:_lib.PNG_HEADER_BYTES]).view(np.int32)
    if hdr.size != 16 or hdr[0] != _lib.PNG_MAGIC:
        raise ValueError("no packed frame")
    return dict(zip(INFO_FIELDS, (int(v) for v in hdr[1:5])))


def batch_geometry(packed_batch):
    """(width, height, channels) of a [N, bytes] batch of packed frames after checking every frame's header and every
    filter byte on the host: the device stage looks at neither.  ValueError for a mixed or damaged batch."""
    if packed_batch.ndim != 2 or packed_batch.dtype != np.uint8 or packed_batch.shape[1] < _lib.PNG_HEADER_BYTES:
        raise ValueError("packed_batch must be uint8 [N, bytes] of packed frames")
    hdr = np.ascontiguousarray(packed_batch[:, :_lib.PNG_HEADER_BYTES]).view(np.int32)
    if np.any(hdr[:, 0] != _lib.PNG_MAGIC):
        raise ValueError("packed_batch: a row is no packed frame")
    if np.any(hdr[:, 1:4] != hdr[:1, 1:4]):
        raise ValueError("packed_batch mixes frames of different geometries (size or channels)")
    width, height, channels = (int(v) for v in hdr[0, 1:4])
    if packed_bytes(width, height, channels) != packed_batch.shape[1]:
        raise ValueError("packed_batch: the rows' length does not match their geometry")
    stride = 1 + width * channels
    if int(packed_batch[:, _lib.PNG_HEADER_BYTES:_lib.PNG_HEADER_BYTES + height * stride:stride].max()) > 4:
        raise ValueError("packed_batch: a scanline's filter byte is above 4")
    return width, height, channels


def _device_stage(packed_d, n, geom, out, dev):
    _lib.call("mr_png_unfilter", _lib.ptr(packed_d), n, *geom, _lib.ptr(out), None, _lib.stream_ptr(dev))


CODEC = framecodec.Codec("frame_png", inflate, packed_info, batch_geometry, 16, _device_stage)  # (16 bytes: magic and geometry)


def unfilter(packed_batch, device):
    """[N, bytes] packed frames of ONE geometry (numpy or CPU tensor) -> uint8 CUDA [N,H,W,3].  One upload, one launch."""
    return framecodec.decode_packed(CODEC, packed_batch, device)


def decode_batch(files, device, threads=None, unsupported="raise"):
    """list of PNG files' bytes (one frame size) -> uint8 CUDA [N,H,W,3].  Inflating runs in ``threads`` threads (default
    min(16, N)); files of one geometry share one upload and one ``unfilter`` call.
    unsupported="raise": a stream the host stage does not support raises NotImplementedError; "pillow": exactly those files
    are decoded by Pillow on the host and their pixels uploaded."""
    return framecodec.decode_batch(CODEC, files, device, threads, unsupported)
