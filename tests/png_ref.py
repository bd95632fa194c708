"""Restatement of the UNFILTER half of a PNG decode as the PNG specification fixes it (section 9: Recon(x) = Filt(x) +
pred(a, b, c) mod 256) and of what ``convert("RGB")`` does with the result (alpha dropped, grey replicated) -- from a packed
frame of ``pngdecode.inflate`` to uint8 [H, W, 3].  The checker of tests/test_png_host.py; tests/test_oracle_png.py pins it
(and the host stage) to the installed Pillow.  Also a small PNG writer that takes the filter type of every row, and the
shared test cases of tests/test_oracle_png.py, tests/test_gpu_png.py and tests/golden/make_golden_png.py."""
import io
import struct
import zlib

import numpy as np

MAGIC, HEADER_BYTES, BAND_ROWS = 0x3150524D, 64, 64
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
COLOR_OF = {1: 0, 3: 2, 2: 4, 4: 6}
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def parse_header(packed):
    hdr = np.frombuffer(np.ascontiguousarray(packed[:HEADER_BYTES]).tobytes(), np.int32)
    assert hdr[0] == MAGIC
    return dict(width=int(hdr[1]), height=int(hdr[2]), channels=int(hdr[3]), color_type=int(hdr[4]))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter_lines(lines, bpp):
    """lines: H filtered scanlines (bytes, the filter byte first) -> uint8 [H, row bytes]; plain Python integers."""
    prev = bytearray(len(lines[0]) - 1)
    rows = []
    for line in lines:
        ft, cur = line[0], bytearray(line[1:])
        for i in range(len(cur)):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
            cur[i] = (cur[i] + pred) & 255
        rows.append(cur)
        prev = cur
    return np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(len(rows), -1)


def to_rgb(samples):
    """[H, W, channels] -> [H, W, 3]: what convert("RGB") gives for L / LA / RGB / RGBA"""
    ch = samples.shape[2]
    return np.ascontiguousarray(samples[:, :, [0, 0, 0]] if ch <= 2 else samples[:, :, :3])


def reconstruct(packed):
    """packed frame (pngdecode.inflate) -> uint8 [H, W, 3]"""
    h = parse_header(packed)
    stride = 1 + h["width"] * h["channels"]
    body = bytes(np.ascontiguousarray(packed[HEADER_BYTES:HEADER_BYTES + h["height"] * stride]))
    lines = [body[y * stride:(y + 1) * stride] for y in range(h["height"])]
    return to_rgb(unfilter_lines(lines, h["channels"]).reshape(h["height"], h["width"], h["channels"]))


# ---- a PNG writer for tests ----------------------------------------------------------------------------------------
def chunk(ctype, payload):
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload))


def filter_lines(samples, filters):
    """samples uint8 [H, W, channels], one filter type per row -> the H filtered scanlines (the encoder's side of section 9)"""
    H, W, bpp = samples.shape
    flat = samples.reshape(H, W * bpp).astype(np.int64)
    lines = []
    for y in range(H):
        cur = flat[y]
        up = flat[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]]) if W * bpp > bpp else np.zeros_like(cur)
        upleft = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]]) if W * bpp > bpp else np.zeros_like(cur)
        ft = int(filters[y])
        if ft == 4:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, upleft)], np.int64)
        else:
            pred = (np.zeros_like(cur), left, up, (left + up) >> 1)[ft]
        lines.append(bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
    return lines


def write_png(lines, width, height, color_type, depth=8, interlace=0, idat_bytes=None, level=6, before_idat=b""):
    """A PNG stream around the given filtered scanlines: IHDR + IDAT (zlib) + IEND with CRCs.  idat_bytes: the size of
    every IDAT chunk's payload (None: one chunk); before_idat: whole chunks placed between IHDR and the first IDAT."""
    z = zlib.compress(b"".join(lines), level)
    step = len(z) if idat_bytes is None else idat_bytes
    idat = b"".join(chunk(b"IDAT", z[i:i + step]) for i in range(0, len(z), step))
    ihdr = struct.pack(">IIBBBBB", width, height, depth, color_type, 0, 0, interlace)
    return SIGNATURE + chunk(b"IHDR", ihdr) + before_idat + idat + chunk(b"IEND", b"")


def make_png(samples, filters, **kw):
    """samples uint8 [H, W, channels] with every row filtered as ``filters`` says -> the stream"""
    H, W, ch = samples.shape
    return write_png(filter_lines(samples, filters), W, H, COLOR_OF[ch], **kw)


def pillow_decode(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- the shared cases: (name, stream builder) -----------------------------------------------------------------------
def content(width, height, channels, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (height, width, channels), dtype=np.uint8)


def smooth(width, height, channels, seed, noise=12):
    """gradient plus noise: what makes an adaptive encoder choose Sub, Up and Paeth"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    base = np.stack([(x * 3 + y * (c + 1) + 40 * c) for c in range(channels)], -1)
    return np.clip(base + rng.integers(-noise, noise + 1, base.shape), 0, 255).astype(np.uint8)


def cycle(height, start=0):
    return [(start + 3 * y) % 5 for y in range(height)]  # (3 is coprime to 5: every filter on consecutive residues)


PAETH_TIES = content(16, 8, 1, 70, 0, 4)     # values 0..3: pa == pb, pb == pc and pa == pb == pc all occur (counted in the tests)
AVERAGE_CARRY = content(9, 6, 3, 71, 200, 256)  # a + b >= 256 everywhere past the first row and column
BAND_HEIGHT = 2 * BAND_ROWS + 3              # the line carried from band to band is used twice
BATCH = ("batch37x29_0", "batch37x29_1", "batch37x29_2")


def hand_cases():
    """name -> (samples [H, W, channels], filters): the streams with forced filters"""
    cases = {}
    for w, h in ((1, 1), (1, 9), (9, 1)):
        for ch in (1, 2, 3, 4):
            cases[f"tiny{w}x{h}_c{ch}"] = (content(w, h, ch, 10 * w + h + ch), cycle(h, ch))
    for ch in (1, 2, 3, 4):
        cases[f"f43120_5x7_c{ch}"] = (content(5, 7, ch, 20 + ch), [4, 3, 1, 2, 0, 4, 3])
    for ft, name in ((4, "paeth"), (3, "average"), (2, "up")):
        cases[f"first_{name}_6x4"] = (content(6, 4, 3, 30 + ft), [ft] + cycle(3, ft))
    cases["paeth_ties_c1"] = (PAETH_TIES, [4] * 8)
    cases["paeth_ties_c3"] = (content(16, 8, 3, 72, 0, 4), [4] * 8)
    cases["average_carry"] = (AVERAGE_CARRY, [3] * 6)
    for h in (63, 64, 65, 257):
        cases[f"h{h}_w5"] = (content(5, h, 3, h), cycle(h, h))
    cases[f"h{BAND_HEIGHT}_w3"] = (content(3, BAND_HEIGHT, 4, 40), cycle(BAND_HEIGHT, 1))
    cases[f"h{BAND_HEIGHT}_w3_paeth"] = (content(3, BAND_HEIGHT, 1, 41), [4] * BAND_HEIGHT)
    for w in (1, 3, 4, 5, 67):
        for ch in (1, 2, 3, 4):
            cases[f"w{w}_h6_c{ch}"] = (content(w, 6, ch, 50 + w + ch), cycle(6, w + ch))
    for k, name in enumerate(BATCH):
        cases[name] = (smooth(37, 29, 3, 60 + k), cycle(29, k))
    return cases


def pillow_cases():
    """name -> (samples, Pillow save options): streams as Pillow's own encoder writes them"""
    cases = {}
    for ch in (1, 2, 3, 4):
        cases[f"pil48x40_c{ch}"] = (smooth(48, 40, ch, 80 + ch), {})
    cases["pil_optimize"] = (smooth(48, 40, 3, 85), dict(optimize=True))
    for level in (0, 1, 9):
        cases[f"pil_level{level}"] = (smooth(37, 29, 3, 86 + level), dict(compress_level=level))
    cases["pil_noise"] = (content(37, 29, 3, 90), {})
    return cases


def pillow_encode(samples, opts):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(samples[:, :, 0] if samples.shape[2] == 1 else samples, MODES[samples.shape[2]]).save(buf, "PNG", **opts)
    return buf.getvalue()


def palette_stream():
    """a palette (colour type 3) stream: what the host stage refuses"""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(smooth(37, 29, 3, 60)).convert("P", palette=Image.Palette.ADAPTIVE, colors=16).save(buf, "PNG")
    return buf.getvalue()


def all_streams():
    """name -> stream, every case (hand-made first)"""
    out = {name: make_png(s, f) for name, (s, f) in hand_cases().items()}
    out.update({name: pillow_encode(s, o) for name, (s, o) in pillow_cases().items()})
    return out
