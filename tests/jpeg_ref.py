"""numpy restatement of the RECONSTRUCTION half of a JPEG decode as libjpeg-turbo does it with its defaults (what Pillow
calls): dequantisation, the islow IDCT (jidctint.c), the range-limit table, fancy chroma upsampling (jdsample.c) and the
YCbCr -> RGB tables (jdcolor.c) -- from a packed frame of ``mr_jpeg_entropy_decode`` to uint8 [H, W, 3].  The checker of
tests/test_gpu_jpeg.py; tests/test_oracle_jpeg.py pins it (and the host stage) to the installed Pillow.  Also the shared
test cases of both, and of tests/golden/make_golden_jpeg.py."""
import io

import numpy as np

MAGIC, HEADER_BYTES = 0x314A524D, 576

# prepare_range_limit_table (jdmaster.c), the part the IDCT indexes with (x & 1023): centred on 128
RANGE_LIMIT = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)]).astype(np.uint8)


def parse_header(packed):
    hdr = np.frombuffer(np.ascontiguousarray(packed[:64]).tobytes(), np.int32)
    assert hdr[0] == MAGIC
    return dict(width=int(hdr[1]), height=int(hdr[2]), ncomp=int(hdr[3]), hl=int(hdr[4]), vl=int(hdr[5]),
                tq=[int(t) for t in hdr[6:9]], restart=int(hdr[9]))


def _idct_pass(d, shift):
    """jpeg_idct_islow's 1-D pass over the first axis of d [8, ...] (int64; the values fit int32 for real streams)."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (d[0] + d[4]) << 13
    tmp1 = (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                     tmp10 - tmp3]) + r >> shift


def idct_blocks(coef, quant):
    """coef [nb, 8, 8] int16 (natural order), quant [8, 8] -> u8 [nb, 8, 8]"""
    d = coef.astype(np.int64) * quant.astype(np.int64)
    ws = _idct_pass(d.transpose(1, 0, 2), 11)              # columns: axis 0 = row index
    out = _idct_pass(ws.transpose(2, 1, 0), 18)            # rows: axis 0 = column index -> [col, nb, row]
    return RANGE_LIMIT[out.transpose(1, 2, 0) & 1023]


def planes(packed):
    """The components' u8 planes, padded to whole MCUs."""
    h = parse_header(packed)
    mx, my = -(-h["width"] // (8 * h["hl"])), -(-h["height"] // (8 * h["vl"]))
    quant = np.frombuffer(np.ascontiguousarray(packed[64:HEADER_BYTES]).tobytes(), np.uint16).reshape(4, 8, 8)
    coef = np.frombuffer(np.ascontiguousarray(packed[HEADER_BYTES:]).tobytes(), np.int16).reshape(-1, 8, 8)
    out, lo = [], 0
    for c in range(h["ncomp"]):
        bw, bh = (mx * h["hl"], my * h["vl"]) if c == 0 else (mx, my)
        px = idct_blocks(coef[lo:lo + bw * bh], quant[h["tq"][c]])
        out.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
        lo += bw * bh
    assert lo == len(coef)
    return h, out


def _h2v1_fancy(p):
    """[rows, n] -> [rows, 2n]"""
    p = p.astype(np.int64)
    prev, nxt = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2_fancy(p):
    """[m, n] real samples -> [2m, 2n]"""
    p = p.astype(np.int64)
    above, below = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for v, other in ((0, above), (1, below)):
        s = 3 * p + other
        prev, nxt = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + prev + 8) >> 4, (3 * s + nxt + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def upsample(plane, h, W, H):
    """A chroma plane at full resolution [H, W]; only the real samples (ceil(W h / hmax) x ceil(H v / vmax)) are read."""
    cw, ch = -(-W // h["hl"]), -(-H // h["vl"])
    p = plane[:ch, :cw]
    if h["hl"] == 2 and h["vl"] == 1:
        p = _h2v1_fancy(p) if cw > 2 else np.repeat(p, 2, 1)
    elif h["hl"] == 2 and h["vl"] == 2:
        p = _h2v2_fancy(p) if cw > 2 else np.repeat(np.repeat(p, 2, 0), 2, 1)
    return p[:H, :W].astype(np.int64)


def reconstruct(packed):
    packed = np.asarray(packed, np.uint8)
    h, pl = planes(packed)
    W, H = h["width"], h["height"]
    y = pl[0][:H, :W].astype(np.int64)
    if h["ncomp"] == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    cb, cr = upsample(pl[1], h, W, H) - 128, upsample(pl[2], h, W, H) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- the shared cases -------------------------------------------------------------------------------------------------
def content(w, h, seed, mode="RGB", checker=False):
    """A deterministic gradient + seeded noise (or a 0 / 255 checkerboard) as uint8 [h, w, 3] (or [h, w] for L)."""
    yy, xx = np.mgrid[0:h, 0:w]
    if checker:
        img = np.repeat((((xx + yy) & 1) * 255)[..., None], 3, 2)
    else:
        rng = np.random.default_rng(seed)
        grad = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], -1)
        img = np.clip(grad + rng.integers(-40, 41, (h, w, 3)), 0, 255)
    img = img.astype(np.uint8)
    return img[..., 0].copy() if mode == "L" else img


GEOMETRIES = ((1, 1), (8, 8), (16, 16), (17, 9), (37, 29), (48, 40))


def case_list():
    """(name, width, height, mode, content seed | 'checker', Pillow save options)"""
    cases = []
    for w, h in GEOMETRIES:
        for sub in (0, 1, 2):
            cases.append((f"g{w}x{h}_s{sub}", w, h, "RGB", 100 * w + h + sub, dict(quality=75, subsampling=sub)))
    cases.append(("grey23x11", 23, 11, "L", 5, dict(quality=75)))
    for q in (5, 100):
        for sub in (0, 2):
            cases.append((f"q{q}_37x29_s{sub}", 37, 29, "RGB", 7 + q, dict(quality=q, subsampling=sub)))
    for sub in (0, 1, 2):
        cases.append((f"checker100_48x40_s{sub}", 48, 40, "RGB", "checker", dict(quality=100, subsampling=sub)))
    cases.append(("optimize_37x29_s2", 37, 29, "RGB", 11, dict(quality=75, subsampling=2, optimize=True)))
    cases.append(("optimize_q100_17x9_s1", 17, 9, "RGB", 12, dict(quality=100, subsampling=1, optimize=True)))
    for rst in (1, 2):
        cases.append((f"rst{rst}_37x29_s2", 37, 29, "RGB", 13 + rst, dict(quality=75, subsampling=2, restart_marker_blocks=rst)))
    # 30 MCUs: the restart markers' numbers wrap around 8
    cases.append(("rst1_48x40_s0", 48, 40, "RGB", 17, dict(quality=75, subsampling=0, restart_marker_blocks=1)))
    cases.append(("rst2_17x9_s2", 17, 9, "RGB", 16, dict(quality=75, subsampling=2, restart_marker_blocks=2)))
    for k, q in enumerate((30, 75, 95)):  # the batch: one geometry, different content AND different tables
        cases.append((f"batch{k}_48x40_s2", 48, 40, "RGB", 20 + k, dict(quality=q, subsampling=2)))
    return cases


BATCH = ("batch0_48x40_s2", "batch1_48x40_s2", "batch2_48x40_s2")
SANITIZER_STREAMS = ("g8x8_s0", "rst2_17x9_s2", "grey23x11")  # the fixtures tests/jpeg_entropy_main.cpp runs over


def encode(case):
    """The case's JPEG stream, encoded by the installed Pillow."""
    from PIL import Image

    name, w, h, mode, seed, opts = case
    img = content(w, h, 0, mode, checker=True) if seed == "checker" else content(w, h, seed, mode)
    buf = io.BytesIO()
    Image.fromarray(img, mode).save(buf, "JPEG", **opts)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
