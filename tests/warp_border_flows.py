"""Flow fields whose samples sit ON and AROUND the image border (a helper module: nothing pytest collects).

``border_flow(B, H, W, seed)`` returns a [B,2,H,W] fp32 flow in which every pixel of the outer two rows and columns -- the four
corners on both axes -- is given a chosen sample position relative to the nearest image side, and the classes it reached:

    on        exactly on the first / last pixel centre (where fp32 reaches it: ``exact`` says so), else the nearest position
    in-band   beyond the centre by 1e-6 .. 8.5e-6: the out-of-bounds weight stays under 1 - 0.99999, the warp mask is 1
    out-band  beyond it by 1.15e-5 .. 3e-5: the mask is 0
    half, one, three   half a pixel, one pixel, three pixels beyond
    big, inf, nan      a flow component of +-1e9, +-inf, NaN

The positions are the ORACLE's: a flow value is found by a search over the neighbouring floats of a first guess, each
candidate evaluated with ``W._vgrid`` and ``W._unnormalize``.  Interior pixels carry random flows of a few pixels.
``check_classes`` is the precondition a test asserts before it launches anything: every class on every side (for images with
fewer border slots than classes: every slot a class, every class somewhere), and no sample whose summed in-bounds weight lies
within 1e-6 of the 0.99999 threshold (the search keeps the bands 1.5e-6 away from it; summation-order noise is 1e-7).
"""
import numpy as np

from oracle import warp_ref as W

F32 = np.float32
CLASSES = ("on", "in-band", "out-band", "half", "one", "three", "big", "inf", "nan")
SIDES = ("L", "R", "T", "B")
THRESH = F32(0.99999)
STEPS = 96  # floats on either side of the first guess


def _positions(size, index, cands, axis):
    """the oracle's unnormalised sample position of pixel ``index`` along ``axis`` (0: x, 1: y) for each candidate flow value"""
    K = len(cands)
    shape = (K, 2, 1, size) if axis == 0 else (K, 2, size, 1)
    flow = np.zeros(shape, F32)
    if axis == 0:
        flow[:, 0, 0, index] = cands
        return W._unnormalize(W._vgrid(flow)[:, 0, index, 0], size)
    flow[:, 1, index, 0] = cands
    return W._unnormalize(W._vgrid(flow)[:, index, 0, 1], size)


def _neighbours(u0):
    out = [F32(u0)]
    lo = hi = F32(u0)
    for _ in range(STEPS):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.array(out, F32)


def flow_for(size, index, high, cls, sign):
    """(flow value, reached position, beyond) for pixel ``index`` of an axis of ``size`` pixels: class ``cls`` at the low
    (``high`` False) or high side; ``beyond``: how far past the side's pixel centre the position is (negative: inside)"""
    edge = float(size - 1) if high else 0.0
    out_dir = 1.0 if high else -1.0
    if cls in ("big", "inf", "nan"):
        u = {"big": F32(1e9), "inf": F32(np.inf), "nan": F32(np.nan)}[cls] * F32(sign if cls != "nan" else 1)
        return u, _positions(size, index, np.array([u], F32), 0)[0], np.nan
    want = {"on": 0.0, "in-band": 6e-6, "out-band": 1.3e-5, "half": 0.5, "one": 1.0, "three": 3.0}[cls]
    target = edge + out_dir * want
    u0 = (target + 0.5) * max(size - 1, 1) / size - index
    cands = _neighbours(u0)
    pos = _positions(size, index, cands, 0).astype(np.float64)
    beyond = (pos - edge) * out_dir
    if cls == "on":
        k = int(np.argmin(np.abs(beyond)))
    elif cls == "in-band":
        ok = (beyond >= 1e-6) & (beyond <= 8.5e-6)
        assert ok.any(), (size, index, high, cls)
        k = int(np.argmax(np.where(ok, beyond, -1)))
    elif cls == "out-band":
        ok = (beyond >= 1.15e-5) & (beyond <= 3e-5)
        assert ok.any(), (size, index, high, cls)
        k = int(np.argmin(np.where(ok, beyond, 1)))
    else:
        k = int(np.argmin(np.abs(beyond - want)))
    return cands[k], pos[k], beyond[k]


def border_flow(B, H, Wd, seed):
    """(flow [B,2,H,W] fp32, reached): reached[(side, class)] = list of (b, y, x, beyond)"""
    rng = np.random.default_rng(seed)
    flow = (rng.standard_normal((B, 2, H, Wd)) * 2).astype(F32)
    reached = {}
    counter = {s: i * 2 for i, s in enumerate(SIDES)}  # (the sides start at different classes: corners mix them)
    for b in range(B):
        for y in range(H):
            for x in range(Wd):
                for axis, (size, idx) in enumerate(((Wd, x), (H, y))):
                    low, high = idx < min(2, (size + 1) // 2), idx >= size - min(2, size // 2)
                    if not (low or high):
                        continue
                    side = (("L", "R"), ("T", "B"))[axis][int(high and not low)]
                    cls = CLASSES[(counter[side] + seed) % len(CLASSES)]
                    counter[side] += 1
                    u, _, beyond = flow_for(size, idx, side in ("R", "B"), cls, 1 if rng.random() < 0.5 else -1)
                    flow[b, axis, y, x] = u
                    reached.setdefault((side, cls), []).append((b, y, x, beyond))
                # the other axis of a side pixel that is no corner: somewhere inside the image
                if not (x < 2 or x >= Wd - 2) and (y < 2 or y >= H - 2):
                    flow[b, 0, y, x] = F32(np.clip(x + rng.uniform(-2, 2), 0.6, Wd - 1.6) - x)
                if not (y < 2 or y >= H - 2) and (x < 2 or x >= Wd - 2):
                    flow[b, 1, y, x] = F32(np.clip(y + rng.uniform(-2, 2), 0.6, H - 1.6) - y)
    return flow, reached


def summed_weight(flow):
    """the oracle's bilinear sample of an all-ones image before it is binarised: [B,H,W]"""
    ones = np.ones((flow.shape[0], 1) + flow.shape[2:], F32)
    return W.grid_sample(ones, W._vgrid(flow))[:, 0]


def check_classes(flow, reached, all_on_every_side=True):
    """the precondition; returns {(side, class): count}"""
    B, _, H, Wd = flow.shape
    counts = {k: len(v) for k, v in reached.items()}
    if all_on_every_side:
        missing = [(s, c) for s in SIDES for c in CLASSES if not counts.get((s, c))]
        assert not missing, f"classes not reached: {missing}"
    else:
        assert {c for _, c in counts} == set(CLASSES) and {s for s, _ in counts} == set(SIDES), counts
    for (side, cls), where in reached.items():
        for b, y, x, beyond in where:
            if cls == "in-band":
                assert 1e-6 <= beyond <= 8.5e-6
            elif cls == "out-band":
                assert 1.15e-5 <= beyond <= 3e-5
            elif cls in ("half", "one", "three"):
                assert abs(beyond - {"half": 0.5, "one": 1.0, "three": 3.0}[cls]) < 1e-4
            elif cls == "on":
                assert abs(beyond) < 1e-5
    acc = summed_weight(flow)
    with np.errstate(invalid="ignore"):
        knife = np.abs(acc.astype(np.float64) - float(THRESH)) < 1e-6
    assert not knife.any(), f"{int(knife.sum())} samples within 1e-6 of the mask threshold"
    # the bands decide the mask as intended where the other axis is inside the image
    mask = W.warp(np.ones((B, 1, H, Wd), F32), flow)[1][:, 0]
    for (side, cls), where in reached.items():
        for b, y, x, _ in where:
            corner = (x < 2 or x >= Wd - 2) and (y < 2 or y >= H - 2)
            if not corner and cls in ("on", "in-band"):
                assert mask[b, y, x] == 1, (side, cls, b, y, x)
            if cls in ("out-band", "half", "one", "three", "big", "inf", "nan"):
                assert mask[b, y, x] == 0, (side, cls, b, y, x)
    return counts
