"""mr_frames_resize (csrc/frame_resize.hip) and the layers above it on a device: Pillow's ``Image.resize(size, BILINEAR)`` of
RGB frames.  The comparison is byte equality everywhere -- no tolerance and no share of pixels left out -- against what the
installed Pillow recorded (tests/golden/resize_pil.npz) and against tests/resize_ref.py's restatement of its arithmetic,
which tests/test_oracle_resize.py holds against Pillow on a CPU.

Cases: every fixture case at N = 1 (the geometries the entry point refuses -- a reduction by more than 16 -- must be refused
from the sizes alone); 37 x 23 <-> 16 x 9 at N = 3 with differing frames; 524 x 268 <-> 131 x 67, outputs that are no
multiple of the tile and span many workgroups; 16 x 16 -> 1 x 1, the tap cap; 20 x 12 -> 20 x 12, the copy; 1920 x 1080 ->
480 x 270 at N = 2 against the restatement and the recorded hash.  Output buffers of the raw calls are pre-filled with a
pattern: a byte nobody writes fails.  Also: two calls give the same bytes; a frame's result does not depend on its batch;
guard bands intact; a non-contiguous input; the call on a side stream behind a delay (tests/test_gpu_side_stream.py's
arrangement) and under one hipGraph capture replayed on changed inputs (tests/test_gpu_graph_replay.py's recipe), since the
host recorder does not link this source; and the dataset chain -- full-size JPEG and PNG files through
``HandObjSet(decode="device", color_fn="device", frame_size=...)`` and ``assemble_batch`` against the host path (both sides
of that comparison need Pillow: the synthetic dataset writes its files with it, as in tests/test_gpu_jpeg.py).

Measured on an MI355X (``RESIZE ...`` lines): 326 fixture cases with zero differing bytes, 112 refused from their sizes; the
side stream's bytes equal the default stream's behind a 19.99 ms delay.  The whole file takes 4 s.
"""
import random

import numpy as np
import pytest
import torch

from tests import resize_ref as R

pytestmark = pytest.mark.gpu


def up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def resize(frames, size):
    from handobjectconsist_amd.datasets import frames as F

    return F.resize(frames, size)


def run_raw(cuda, src, size, fill=0xA5):
    """the entry point as it is, with freshly built tables, on a pattern-filled output -> uint8 numpy [N,H,W,3]"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import frames as F

    N, Hs, Ws, _ = src.shape
    W, H = size
    tabs = [up(t, cuda) for t in F.resize_tables(Ws, W) + F.resize_tables(Hs, H)]
    out = torch.full((N, H, W, 3), fill, dtype=torch.uint8, device=cuda)
    assert _lib.load().mr_frames_resize_workspace_bytes(N, Ws, Hs, W, H) == 0
    _lib.call("mr_frames_resize", _lib.ptr(up(src, cuda)), N, Ws, Hs, _lib.ptr(out), W, H, *[_lib.ptr(t) for t in tabs], None,
              _lib.stream_ptr(cuda))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def differing(got, want):
    return int((np.asarray(got) != np.asarray(want)).sum())


# ---- values -----------------------------------------------------------------------------------------------------------------------
def test_every_fixture_case(cuda):
    """N = 1, against Pillow's recorded bytes (its SHA-256 where the fixture holds only that)"""
    meta, arrays = R.load_fixture()
    assert len(meta) == len(R.cases())
    ran = refused = 0
    for m in meta:
        g = tuple(m["geometry"])
        src = R.contents(m["kind"], m["seed"], g[0], g[1])
        if not R.supported(g):
            with pytest.raises(NotImplementedError):
                resize(up(src, cuda), g[2:])
            refused += 1
            continue
        got = resize(up(src, cuda), g[2:]).cpu().numpy()
        assert got.shape == (1, g[3], g[2], 3) and got.dtype == np.uint8
        if "sha256" in m:
            assert R.sha256(got[0]) == m["sha256"], m["key"]
        else:
            assert differing(got[0], arrays[m["key"]]) == 0, (m["key"], differing(got[0], arrays[m["key"]]))
        ran += 1
    print(f"RESIZE fixture: {ran} cases with zero differing bytes, {refused} refused from their sizes")
    assert ran >= 300 and refused == len(meta) - ran


BATCHED = [((37, 23, 16, 9), 3), ((16, 9, 37, 23), 3), ((524, 268, 131, 67), 2), ((131, 67, 524, 268), 2), ((16, 16, 1, 1), 3),
           ((20, 12, 20, 12), 2), ((64, 36, 16, 36), 2), ((36, 64, 36, 16), 2),
           ((1700, 40, 107, 5), 2)]  # (a strip of 525 columns, staged 10 rows at a time: four chunks a tile)


@pytest.mark.parametrize("geom,n", BATCHED, ids=lambda v: "%dx%d-%dx%d" % v if isinstance(v, tuple) else f"N{v}")
@pytest.mark.parametrize("kind", ["uniform", "binary"])
def test_batches_against_the_restatement(cuda, geom, n, kind):
    """differing frames; the raw entry point on a pattern-filled output and the Python layer; a second call has the same
    bytes; each frame equals its own N = 1 call"""
    src = R.contents(kind, 11, geom[0], geom[1], frames=n)
    assert differing(src[0], src[1]) > 0
    want = R.resize(src, geom[2:])
    raw = run_raw(cuda, src, geom[2:])
    assert differing(raw, want) == 0, differing(raw, want)
    assert differing(run_raw(cuda, src, geom[2:], fill=0x5A), want) == 0, "a byte nobody writes"
    src_d = up(src, cuda)
    got = resize(src_d, geom[2:])
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and got.data_ptr() != src_d.data_ptr()
    assert differing(got.cpu().numpy(), want) == 0
    assert torch.equal(resize(src_d, geom[2:]), got), "two calls differ"
    for k in range(n):
        assert torch.equal(resize(src_d[k:k + 1], geom[2:]), got[k:k + 1]), f"frame {k} alone differs"


def test_full_hd_to_quarter_size(cuda):
    """1920 x 1080 -> 480 x 270 at N = 2: frame 0 is the fixture's (Pillow's recorded hash), frame 1 against the restatement"""
    meta, _ = R.load_fixture()
    m = next(m for m in meta if tuple(m["geometry"]) == R.LARGE and m["kind"] == "uniform")
    src = np.concatenate([R.contents("uniform", m["seed"], 1920, 1080), R.contents("binary", 9, 1920, 1080)])
    got = resize(up(src, cuda), (480, 270)).cpu().numpy()
    assert got.shape == (2, 270, 480, 3)
    assert R.sha256(got[0]) == m["sha256"]
    want = R.resize(src[1], (480, 270))
    assert differing(got[1], want) == 0, differing(got[1], want)
    assert differing(run_raw(cuda, src[1:], (480, 270))[0], want) == 0


def test_empty_batch_and_refusals(cuda):
    empty = resize(torch.zeros((0, 23, 37, 3), dtype=torch.uint8, device=cuda), (16, 9))
    assert tuple(empty.shape) == (0, 9, 16, 3)
    frames = up(R.contents("uniform", 1, 40, 33), cuda)
    with pytest.raises(NotImplementedError):
        resize(frames, (40, 2))   # 33 -> 2: 35 taps
    with pytest.raises(NotImplementedError):
        resize(frames, (10753, 4))
    with pytest.raises(ValueError):
        resize(frames, (0, 4))
    with pytest.raises(ValueError):
        resize(frames.float(), (4, 4))
    with pytest.raises(ValueError):
        resize(frames[0], (4, 4))
    assert not resize(frames, (20, 11)).requires_grad


def test_tables_are_cached_by_value(cuda):
    from handobjectconsist_amd.datasets import frames as F

    F._RESIZE_TABLES.clear()
    a = up(R.contents("uniform", 2, 37, 23), cuda)
    resize(a, (16, 9))
    resize(a.clone(), [16, 9])
    resize(up(R.contents("uniform", 3, 37, 23, frames=2), cuda), (np.int64(16), 9))
    assert list(F._RESIZE_TABLES) == [(37, 23, 16, 9, "cuda", 0)]
    resize(a, (9, 16))
    assert len(F._RESIZE_TABLES) == 2


# ---- memory -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(37, 23, 16, 9), (524, 268, 131, 67)], ids=lambda g: "%dx%d-%dx%d" % g)
def test_guard_bands(cuda, monkeypatch, geom):
    """input, output and the four tables inside guard bands: no band changes, every pointer the entry point gets lies inside
    a guarded interior, and the bytes are those of the plain run"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import frames as F
    from tests import guarded_alloc as G

    src = up(R.contents("uniform", 4, geom[0], geom[1], frames=2), cuda)
    plain = resize(src, geom[2:])
    torch.cuda.synchronize()
    alloc = G.GuardedAllocator(cuda)
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append((n, a)), real_call(n, *a))[1])
    F._RESIZE_TABLES.clear()  # (the tables are then built, and guarded, inside)
    alloc.install(monkeypatch)
    try:
        got = resize(alloc.guard(src), geom[2:])
        damage = alloc.check()
    finally:
        alloc.uninstall()
        monkeypatch.setattr(_lib, "call", real_call)
        F._RESIZE_TABLES.clear()
    strangers = alloc.pointer_report(calls)
    print(f"RESIZE guard bands {geom}: {alloc.count()} guarded allocations, {alloc.pointers_seen} pointer arguments")
    assert not damage, "\n".join(damage)
    assert not strangers, strangers
    assert [n for n, _ in calls] == ["mr_frames_resize"] and alloc.pointers_seen == 6
    assert alloc.holds(got) and torch.equal(got, plain)


def test_non_contiguous_input(cuda):
    src = R.contents("uniform", 6, 37, 23, frames=3)
    want = R.resize(src, (16, 9))
    wide = torch.full((3, 25, 40, 3), 255, dtype=torch.uint8, device=cuda)
    wide[:, 1:24, 2:39] = up(src, cuda)
    view = wide[:, 1:24, 2:39]                                              # an offset view with padded rows
    chw = up(src, cuda).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)  # [N,H,W,3] over [N,3,H,W] memory
    every_other = up(np.repeat(src, 2, axis=0), cuda)[::2]
    for what, t in (("offset view", view), ("permuted", chw), ("strided batch", every_other)):
        assert not t.is_contiguous(), what
        assert differing(resize(t, (16, 9)).cpu().numpy(), want) == 0, what
    assert torch.equal(resize(view, (37, 23)), up(src, cuda)) and resize(view, (37, 23)).is_contiguous(), "the copy of a view"
    # dense frames that begin at an odd address: the entry point asks no alignment of frames_in
    for shift in (1, 2, 3):
        buf = torch.full((src.size + 8,), 255, dtype=torch.uint8, device=cuda)
        odd = buf[shift:shift + src.size].view(src.shape)
        odd.copy_(up(src, cuda))
        assert odd.is_contiguous() and odd.data_ptr() % 4 == shift
        assert differing(resize(odd, (16, 9)).cpu().numpy(), want) == 0, f"frames at an address = {shift} mod 4"


# ---- streams ----------------------------------------------------------------------------------------------------------------------
from tests.test_gpu_side_stream import delay  # noqa: E402,F401  (the session's calibrated delay, as that file measures it)


def test_side_stream_behind_a_delay(cuda, delay):  # noqa: F811
    """the frames arrive on a side stream after a 20 ms delay kernel: a launch on any other stream would read the stale zeros"""
    from tests import test_gpu_side_stream as SS

    geom = (524, 268, 131, 67)
    src = R.contents("uniform", 8, geom[0], geom[1], frames=2)
    resize(up(src, cuda), geom[2:])  # (the tables are built and cached before the streams part)
    side = SS.run_family(delay, f"frames.resize {geom}", [up(src, cuda)], lambda f: [resize(f, geom[2:])], ["frames"], [SS.EXACT])
    assert differing(side[0].cpu().numpy(), R.resize(src, geom[2:])) == 0


def test_graph_replay(cuda):
    """one capture, replayed twice on changed frames: the eager call's bytes each time"""
    from tests.test_gpu_graph_replay import capture

    geom = (524, 268, 131, 67)
    sets = [up(R.contents(kind, seed, geom[0], geom[1], frames=2), cuda) for kind, seed in (("uniform", 1), ("binary", 2), ("uniform", 3))]
    eager = [resize(s, geom[2:]) for s in sets]
    torch.cuda.synchronize()
    assert not torch.equal(eager[1], eager[2])
    static = sets[0].clone()
    graph, side, out = capture(lambda: resize(static, geom[2:]))
    torch.cuda.synchronize()
    for k in (1, 2):
        static.copy_(sets[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k]), f"replay {k} differs from the eager call on the same frames"


# ---- the dataset chain ------------------------------------------------------------------------------------------------------------
SIZE = (160, 90)


@pytest.mark.parametrize("fmt", [dict(jpeg_quality=90), dict(png_compress_level=1)], ids=["jpeg", "png"])
def test_dataset_chain_equals_the_host_path(cuda, fmt):
    """640 x 360 files of a dataset annotated at 160 x 90, train mode with mirrored samples: packed frames -> device decode ->
    ``frames.resize`` -> device colour augmentation -> batch, against Pillow's decode, resize, blur and jitter on the host,
    on the same RNG streams -- bit for bit in ``image`` and ``jittermask``"""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.datasets import handobjset, synthpose
    from handobjectconsist_amd.utils import collate

    batches = {}
    for decode, color_fn in (("host", "reference"), ("device", "device")):
        ds = synthpose.SynthPoseDataset(num_pairs=2, frame_size=SIZE, seed=1, sides=("right", "left"), file_scale=4, **fmt)
        hs = handobjset.HandObjSet(ds, inp_res=(64, 64), color_fn=color_fn, decode=decode, sample_nb=2, sides="right", frame_size=SIZE)
        random.seed(21)
        torch.manual_seed(21)
        batches[decode] = collate.seq_extend_collate([hs[i] for i in (0, 3)], ["objverts3d", "objfaces", "objcanverts"])
    host, dev = batches["host"], batches["device"]
    key = "frame_jpeg" if "jpeg_quality" in fmt else "frame_png"
    assert all(key in d and "frame" not in d and d["resize_to"].tolist() == [list(SIZE)] * 2 for d in dev)
    assert all(tuple(d["frame"].shape) == (2, 90, 160, 3) and "resize_to" not in d for d in host)
    assert any(bool(d["flip"].any()) for d in dev) and not all(bool(d["flip"].all()) for d in dev)
    calls = []
    real_call = _lib.call
    _lib.call = lambda n, *a: (calls.append(n), real_call(n, *a))[1]
    try:
        b = handobjset.assemble_batch(dev, cuda, (64, 64))
    finally:
        _lib.call = real_call
    assert calls.count("mr_frames_resize") == 1 and calls.index("mr_frames_resize") < calls.index("mr_frames_color_augment")
    a = handobjset.assemble_batch(host, cuda, (64, 64))
    for fa, fb in zip(a, b):
        assert "resize_to" not in fb and key not in fb and fa.keys() == fb.keys()
        assert fa["image"].shape == (2, 3, 64, 64) and torch.equal(fa["image"], fb["image"])
        assert torch.equal(fa["jittermask"], fb["jittermask"])
        assert float(fa["jittermask"].float().mean()) > 0.2, "the crops miss the frames"
