"""The host side of the frame resize (csrc/resize_plan.hpp through the C-ABI, datasets/frames.py, datasets/handobjset.py,
scripts/reduce_frames.py) on a machine without a GPU.

* ``mr_frames_resize_tables`` equals tests/resize_ref.py's restatement of Pillow's tables integer for integer -- every
  (in, out) in 1..48 and the large axes 1920 -> 480, 1080 -> 270, 640 -> 480, 10752 -> 672, 16 -> 1 --, ``taps`` matches, and
  the refusals carry the documented codes.
* The plan's invariants over the same sweep (as heights, and as widths) and the large geometries: LDS within 65536 bytes and
  as the kernel lays it out, the tiles cover the output exactly once, and for every tile the rows it holds include every row
  its ``bounds_y`` entries name -- and the columns it stages every column its ``bounds_x`` entries name.
* ``mr_frames_resize`` validates its arguments before it touches a device.
* ``HandObjSet(frame_size=...)`` on the host path is Pillow's resize followed by the existing path on the resized frames, on
  identical draws; files of the stated size give identical samples; a mixed batch is a ValueError; the reduction tool's walk
  and batching with Pillow injected as the resize."""
import ctypes
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE_AXES = ((1920, 480), (1080, 270), (640, 480), (10752, 672), (16, 1))
LARGE_GEOMETRIES = ((1920, 1080, 480, 270), (640, 480, 480, 270), (10752, 10752, 672, 672), (16, 16, 1, 1), (480, 270, 1920, 1080),
                    (10752, 1080, 672, 270))
BADARG, NOTIMPL = -1, -2


def lib():
    from handobjectconsist_amd import _lib

    return _lib.load()


def c_tables(in_size, out_size):
    from handobjectconsist_amd.datasets import frames

    return frames.resize_tables(in_size, out_size)


def c_plan(geom):
    from handobjectconsist_amd import _lib

    plan = (ctypes.c_int * (_lib.RESIZE_PLAN_INTS + 1))(*([-7] * (_lib.RESIZE_PLAN_INTS + 1)))
    rc = lib().mr_frames_resize_plan(*geom, plan)
    assert plan[_lib.RESIZE_PLAN_INTS] == -7, "the plan is RESIZE_PLAN_INTS long"
    return rc, dict(zip(("tile_w", "tile_h", "rows", "lds", "grid_x", "grid_y", "cols", "chunk_rows"), plan))


# ---- tables -------------------------------------------------------------------------------------------------------------------
def test_tables_equal_the_restatement_integer_for_integer():
    axes = [(i, o) for i in range(1, 49) for o in range(1, 49)] + list(LARGE_AXES)
    checked = refused = 0
    for in_size, out_size in axes:
        taps = lib().mr_frames_resize_taps(in_size, out_size)
        if R.taps_of(in_size, out_size) > 33:
            assert taps == NOTIMPL, (in_size, out_size)
            with pytest.raises(NotImplementedError):
                c_tables(in_size, out_size)
            refused += 1
            continue
        assert taps == R.taps_of(in_size, out_size), (in_size, out_size)
        bounds, coeffs = c_tables(in_size, out_size)
        want_b, want_c = R.tables(in_size, out_size)
        assert coeffs.shape == (out_size, taps) and np.array_equal(bounds, want_b), (in_size, out_size)
        assert np.array_equal(coeffs, want_c), (in_size, out_size)
        checked += 1
    assert refused == sum(1 for i, o in axes if i > 16 * o) > 0 and checked + refused == len(axes)


def test_an_axis_that_keeps_its_size_is_the_identity_table():
    for n in (1, 2, 7, 480):
        bounds, coeffs = c_tables(n, n)
        assert coeffs.shape == (n, 3) and np.array_equal(bounds[:, 0], np.arange(n))
        assert np.all(coeffs[:, 0] == 1 << 22) and not coeffs[:, 1:].any()


def test_refusals_carry_the_documented_codes():
    L = lib()
    assert L.mr_frames_resize_taps(16, 1) == 33 and L.mr_frames_resize_taps(33, 1) == NOTIMPL
    assert L.mr_frames_resize_taps(10752, 672) == 33 and L.mr_frames_resize_taps(10753, 10753) == NOTIMPL
    assert L.mr_frames_resize_taps(8, 10753) == NOTIMPL and L.mr_frames_resize_taps(1, 10752) == 3
    assert L.mr_frames_resize_taps(0, 4) == BADARG and L.mr_frames_resize_taps(4, 0) == BADARG and L.mr_frames_resize_taps(-1, 10753) == BADARG
    buf = (ctypes.c_int * 256)()
    assert L.mr_frames_resize_tables(33, 1, buf, buf) == NOTIMPL and L.mr_frames_resize_tables(0, 1, buf, buf) == BADARG
    assert L.mr_frames_resize_tables(4, 2, None, buf) == BADARG and L.mr_frames_resize_tables(4, 2, buf, None) == BADARG
    assert L.mr_frames_resize_plan(33, 8, 1, 8, buf) == NOTIMPL and L.mr_frames_resize_plan(8, 33, 8, 1, buf) == NOTIMPL
    assert L.mr_frames_resize_plan(10753, 8, 8, 8, buf) == NOTIMPL and L.mr_frames_resize_plan(8, 8, 8, 0, buf) == BADARG
    assert L.mr_frames_resize_plan(8, 8, 8, 8, None) == BADARG
    assert L.mr_frames_resize_workspace_bytes(4, 1920, 1080, 480, 270) == 0 and L.mr_frames_resize_workspace_bytes(0, 8, 8, 8, 8) == 0
    assert L.mr_frames_resize_workspace_bytes(-1, 8, 8, 8, 8) == BADARG and L.mr_frames_resize_workspace_bytes(1, 33, 8, 1, 8) == NOTIMPL


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def check_plan(geom):
    src_w, src_h, dst_w, dst_h = geom
    rc, p = c_plan(geom)
    assert rc == 0, geom
    again = c_plan(geom)
    assert again == (rc, p), "the plan is a pure function of the sizes"
    tx, ty = R.taps_of(src_w, dst_w), R.taps_of(src_h, dst_h)
    assert p["tile_w"] == 32 and p["tile_h"] in (1, 2, 4, 8, 16), (geom, p)
    strip_pitch = (3 * p["cols"] + 15 + 15) & ~15  # a staged row: its columns' bytes behind up to 15 bytes of its first 16
    assert 1 <= p["chunk_rows"] <= p["rows"] and (p["chunk_rows"] == p["rows"] or p["chunk_rows"] >= 8), (geom, p)
    assert 0 < p["lds"] <= 65536, (geom, p)
    tables = (4 * (32 * tx + p["tile_h"] * ty) + 15) & ~15
    assert p["lds"] == tables + 96 * p["rows"] + p["chunk_rows"] * strip_pitch + 64, (geom, p)
    # a regular grid of tiles: it covers the output exactly once when the last tile of each axis begins inside the output
    for n_tiles, tile, out in ((p["grid_x"], p["tile_w"], dst_w), (p["grid_y"], p["tile_h"], dst_h)):
        assert (n_tiles - 1) * tile < out <= n_tiles * tile, (geom, p)
    assert p["grid_y"] <= 65535
    by, _ = R.tables(src_h, dst_h)
    for t in range(p["grid_y"]):
        rows = by[t * p["tile_h"]:min((t + 1) * p["tile_h"], dst_h)]
        first = int(rows[0, 0])  # what the kernel takes as the tile's first row
        assert int(rows[:, 0].min()) == first and int((rows[:, 0] + rows[:, 1]).max()) - first <= p["rows"], (geom, t, p)
    assert 1 <= p["rows"] <= src_h
    bx, _ = R.tables(src_w, dst_w)  # ... and the columns it stages include every column its bounds_x entries name
    for t in range(p["grid_x"]):
        cols = bx[t * 32:min((t + 1) * 32, dst_w)]
        first = int(cols[0, 0])
        assert int(cols[:, 0].min()) == first and int((cols[:, 0] + cols[:, 1]).max()) - first <= p["cols"], (geom, t, p)
    assert 1 <= p["cols"] <= src_w
    return p


def test_plan_invariants():
    for i in range(1, 49):
        for o in range(1, 49):
            if R.taps_of(i, o) <= 33:
                check_plan((20, i, 20, o))  # the sweep as heights ...
                check_plan((i, 9, o, 4))    # ... and as widths
    plans = {g: check_plan(g) for g in LARGE_GEOMETRIES}
    assert plans[(16, 16, 1, 1)]["rows"] == 16 and plans[(1920, 1080, 480, 270)]["tile_h"] == 16
    assert plans[(10752, 10752, 672, 672)]["tile_h"] < 16, "a lower tile for large factors"


# ---- the launcher's checks ------------------------------------------------------------------------------------------------------
def test_argument_validation_needs_no_device():
    L = lib()
    ok = dict(frames_in=0x1000, num_frames=2, src_w=37, src_h=23, frames_out=0x2000, dst_w=16, dst_h=9, bounds_x=0x3000,
              coeffs_x=0x4000, bounds_y=0x5000, coeffs_y=0x6000, workspace=None, stream=None)

    def call(**over):
        return L.mr_frames_resize(*dict(ok, **over).values())

    for name in ("frames_in", "frames_out", "bounds_x", "coeffs_x", "bounds_y", "coeffs_y"):
        assert call(**{name: None}) == BADARG, name
        assert call(**{name: None}, num_frames=0) == 0, name  # an empty batch touches nothing
    for name in ("frames_out", "bounds_x", "coeffs_x", "bounds_y", "coeffs_y"):
        assert call(**{name: ok[name] + 2}) == BADARG, name
    for name in ("src_w", "src_h", "dst_w", "dst_h"):
        assert call(**{name: 0}) == BADARG and call(**{name: -3}, num_frames=0) == BADARG, name
        assert call(**{name: 10753}) == NOTIMPL, name
    assert call(num_frames=-1) == BADARG
    assert call(src_w=33, dst_w=1) == NOTIMPL and call(src_h=33, dst_h=1) == NOTIMPL
    assert call(src_w=0, frames_in=None) == BADARG


def test_python_layer_refuses_before_any_launch():
    from handobjectconsist_amd.datasets import frames

    with pytest.raises(TypeError):
        frames.resize(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2))  # (a CPU tensor)
    with pytest.raises(NotImplementedError, match="BILINEAR"):
        frames.resize(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2), resample=3)


# ---- the dataset ------------------------------------------------------------------------------------------------------------------
class Resized:
    """a pose dataset whose ``get_image`` hands out Pillow's resize of another's: the reference of the host path"""

    def __init__(self, ds, size):
        self.ds, self.size = ds, size

    def __len__(self):
        return len(self.ds)

    def __getattr__(self, name):
        return getattr(self.ds, name)

    def get_image(self, idx):
        from PIL import Image

        return np.asarray(Image.fromarray(np.asarray(self.ds.get_image(idx))).resize(self.size, Image.BILINEAR))


def same(a, b, path="sample"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (path, list(a), list(b))
        for k in a:
            same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif a is None or isinstance(a, (str, bool)):
        assert a == b and type(a) is type(b), path
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), path


def draw(hs, idxs=(0, 3, 2)):
    random.seed(5)
    torch.manual_seed(5)
    out = [hs[i] for i in idxs]
    return out, torch.rand(1).item()  # (... and where the RNG stream stands afterwards)


SIZE = (80, 45)


@pytest.mark.parametrize("fmt", [dict(), dict(jpeg_quality=90), dict(png_compress_level=1)], ids=["arrays", "jpeg", "png"])
def test_host_path_is_pillows_resize_in_front_of_the_existing_path(fmt):
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=SIZE, seed=3, sides=("right", "left"), file_scale=4, **fmt)
    assert np.asarray(ds.get_image(0)).shape == (180, 320, 3)
    kw = dict(inp_res=(32, 32), sample_nb=2, sides="right")
    got, rng_got = draw(handobjset.HandObjSet(ds, frame_size=SIZE, **kw))
    want, rng_want = draw(handobjset.HandObjSet(Resized(ds, SIZE), **kw))
    same(got, want)
    assert rng_got == rng_want
    assert got[0][0]["frame"].shape == (45, 80, 3) and any(s["flip"] for seq in got for s in seq)
    plain, _ = draw(handobjset.HandObjSet(ds, **kw))  # without frame_size the full-size frame travels
    assert plain[0][0]["frame"].shape == (180, 320, 3)


@pytest.mark.parametrize("decode", ["host", "device"])
def test_files_of_the_stated_size_change_nothing(decode):
    from handobjectconsist_amd.datasets import handobjset, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=SIZE, seed=3, sides=("right", "left"), png_compress_level=1)
    kw = dict(inp_res=(32, 32), sample_nb=2, sides="right", decode=decode, color_fn="device")
    got, rng_got = draw(handobjset.HandObjSet(ds, frame_size=SIZE, **kw))
    want, rng_want = draw(handobjset.HandObjSet(ds, **kw))
    same(got, want)
    assert rng_got == rng_want and not any("resize_to" in s for seq in got for s in seq)


def test_device_decode_carries_the_file_as_it_is_and_the_target():
    from handobjectconsist_amd.datasets import handobjset, pngdecode, synthpose

    ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=SIZE, seed=3, sides=("right", "left"), file_scale=4, png_compress_level=1)
    kw = dict(inp_res=(32, 32), sample_nb=2, sides="right", color_fn="device", frame_size=SIZE)
    dev, rng_dev = draw(handobjset.HandObjSet(ds, decode="device", **kw))
    host, rng_host = draw(handobjset.HandObjSet(ds, decode="host", **kw))
    assert rng_dev == rng_host
    for sd, sh in zip((s for seq in dev for s in seq), (s for seq in host for s in seq)):
        assert np.array_equal(sd["resize_to"], SIZE) and sd["resize_to"].dtype == np.int32 and "frame" not in sd
        assert pngdecode.packed_info(sd["frame_png"])["width"] == 320
        assert set(sd) - {"frame_png", "resize_to"} == set(sh) - {"frame"}
        for k in set(sh) - {"frame"}:  # the mirror width is frame_size's in both modes: the same centres and affines
            same(sd[k], sh[k], k)


def test_assemble_batch_refuses_a_mixed_batch():
    from handobjectconsist_amd.datasets import handobjset

    def frame_dict(resize_to):
        d = {"frame": torch.zeros(2, 8, 8, 3, dtype=torch.uint8), "affinetrans": torch.eye(3).repeat(2, 1, 1), "flip": torch.zeros(2, dtype=torch.bool)}
        if resize_to is not None:
            d["resize_to"] = torch.tensor([resize_to, resize_to], dtype=torch.int32)
        return d

    with pytest.raises(ValueError, match="resize_to in 1 of 2"):
        handobjset.assemble_batch([frame_dict((4, 4)), frame_dict(None)], "cpu", (8, 8))
    with pytest.raises(ValueError, match="different sizes"):
        handobjset.assemble_batch([frame_dict((4, 4)), frame_dict((4, 2))], "cpu", (8, 8))


# ---- the reduction tool -------------------------------------------------------------------------------------------------------------
def test_reduce_tree_walks_batches_and_skips(tmp_path):
    from PIL import Image

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import reduce_frames
    finally:
        sys.path.pop(0)

    src, dst = tmp_path / "src", tmp_path / "dst"
    rng = np.random.default_rng(0)
    files = {}
    for k, (rel, size) in enumerate([("a/color/0.jpeg", (64, 36)), ("a/color/1.jpeg", (64, 36)), ("a/color/2.jpeg", (64, 36)),
                                      ("b/x/0.png", (64, 36)), ("b/x/1.png", (40, 30)), ("b/x/2.jpeg", (40, 30)), ("top.JPG", (64, 36))]):
        path = src / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(path)
        files[rel] = size
    (src / "a" / "notes.txt").write_text("not a frame")
    (dst / "a" / "color").mkdir(parents=True)
    (dst / "a" / "color" / "1.jpeg").write_bytes(b"already here")

    calls = []

    def pillow_reduce(datas, size):
        ims = [Image.open(io.BytesIO(d)) for d in datas]
        calls.append((ims[0].format, ims[0].size, len(datas)))
        assert len({(im.format, im.size) for im in ims}) == 1, "a group is one format and geometry"
        return np.stack([np.asarray(im.convert("RGB").resize(size, Image.BILINEAR)) for im in ims])

    stats = reduce_frames.reduce_tree(str(src), str(dst), (16, 9), pillow_reduce, batch=2)
    assert stats == {"written": 6, "skipped": 1, "groups": 5}, stats
    # JPEG 64 x 36: a/color/0, a/color/2 fill a batch of 2; top.JPG is flushed at the end
    assert sorted(calls) == sorted([("JPEG", (64, 36), 2), ("JPEG", (64, 36), 1), ("PNG", (64, 36), 1), ("PNG", (40, 30), 1), ("JPEG", (40, 30), 1)])
    assert (dst / "a" / "color" / "1.jpeg").read_bytes() == b"already here"
    for rel in files:
        if rel == "a/color/1.jpeg":
            continue
        with Image.open(src / rel) as im:
            want = io.BytesIO()
            im.resize((16, 9), Image.BILINEAR).save(want, format=im.format)  # the reference: resize, save with defaults
        assert (dst / rel).read_bytes() == want.getvalue(), rel
    assert not [p for p in dst.rglob("*") if p.name.startswith(".part-")] and not (dst / "a" / "notes.txt").exists()
    again = reduce_frames.reduce_tree(str(src), str(dst), (16, 9), pillow_reduce, batch=2)
    assert again == {"written": 0, "skipped": 7, "groups": 0}
