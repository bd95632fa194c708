"""The stem convolution's weight gradient from the pooled records (``mr_stem_conv_wrw``, csrc/stem_wrw.hip) and the
sums-only form of the records backward (``mr_stem_pool_param_grads``).

Reference for the weight gradient: ``torch.nn.grad.conv2d_weight`` on the CPU in fp64 over the gradient map G that the
existing layout-2 ``mr_stem_pool_backward`` writes, cast to fp32.

Exact cases: image integers in [-4, 4], pooled gradients integers in [-2, 2] (two of them: |g + g2| <= 4), a in
{0.5, 1, 2} with both signs and biases around zero so that z = d * a + b takes both signs.  |G| <= 4 windows * 4 * 2 = 32
in steps of 0.5, a product is at most 128 and the largest case sums 8 * 131 * 49 = 51352 of them: below 2^24 halves, so
every product and every partial sum is exact in fp32 in any order and the kernel must match the reference bit for bit.

Random data: both the new kernel and the composed path (the same map through torch's GPU ``conv2d_weight``) are fp32 sums
of the same terms in different orders; the new kernel's largest error against fp64, relative to max |gW|, may be at most
twice the composed path's at the same shape (a margin over the yardstick, not a property of the kernel).

Every device buffer comes from tests/guarded_alloc.py, whose bands catch stores past an end and whose 0xFF fill turns an
over-read that is used into a NaN."""
import ctypes
import functools

import pytest
import torch

from tests import guarded_alloc as G

pytestmark = pytest.mark.gpu

C = 64
EPS = 2.0 ** -10
VAR = 0.25 - EPS  # var + eps = 0.25 exactly, invstd = 2


def _tiling():
    from handobjectconsist_amd import _lib

    ty, tx, wg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.load().mr_stem_conv_wrw_tiling(ctypes.byref(ty), ctypes.byref(tx), ctypes.byref(wg)) == 0
    return ty.value, tx.value, wg.value


def _tile_shape():
    """more than one tile in both directions, no multiple of the tile, and more tiles than workgroups: some workgroups
    take two tiles.  Two tile columns, 8 images, as many tile rows as that needs."""
    ty, tx, wg = _tiling()
    conv_w = tx + tx // 2 + 1
    rows = wg // (2 * 8) + 1
    conv_h = rows * ty - 1
    assert 8 * rows * 2 > wg and conv_h > ty and conv_h % ty and conv_w % tx
    return (8, 2 * conv_h, 2 * conv_w)


SMALL = [(1, 8, 8),      # conv 4 x 4, pooled 2 x 2: one tile, all other workgroups write zero partials
         (2, 22, 18),    # conv 11 x 9, both odd: clipped windows at the right and bottom
         (2, 23, 19),    # odd image: the convolution's floor
         (3, 36, 70)]    # two tile columns
SHAPES = SMALL + ["tiles"]


def _shape(s):
    return _tile_shape() if s == "tiles" else s


def _dims(shape):
    N, Hin, Win = shape
    H, W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
    return N, Hin, Win, H, W, (H - 1) // 2 + 1, (W - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def _inputs(shape, exact):
    """CPU tensors: image [N,3,Hin,Win], x [N,C,H,W] (stands for the convolution's output: the records come from it),
    two pooled gradients, bn weight / bias / mean"""
    N, Hin, Win, H, W, OH, OW = _dims(shape)
    g = torch.Generator().manual_seed(1000 * N + 10 * Hin + Win + (1 if exact else 0))
    if exact:
        ints = lambda s, lo, hi: torch.randint(lo, hi + 1, s, generator=g).float()
        a = torch.tensor([0.5, 1.0, 2.0, -0.5, -1.0, -2.0])[torch.randint(0, 6, (C,), generator=g)]
        return (ints((N, 3, Hin, Win), -4, 4), ints((N, C, H, W), -4, 4), ints((N, C, OH, OW), -2, 2),
                ints((N, C, OH, OW), -2, 2), a / 2, ints((C,), -2, 2), ints((C,), -1, 1))
    rn = lambda *s: torch.randn(*s, generator=g)
    return (rn(N, 3, Hin, Win), rn(N, C, H, W), rn(N, C, OH, OW), rn(N, C, OH, OW), 0.5 + torch.rand(C, generator=g),
            0.3 * rn(C), 0.3 * rn(C))


class Run:
    """One guarded run of the existing layout-2 forward + backward (records, the gradient map G, the BatchNorm gradients)
    and of the two new entry points on the same inputs."""

    def __init__(self, cuda, monkeypatch, shape, exact, gy=None, gy2="default", weight_cl=True, repeat=False):
        from handobjectconsist_amd import _lib

        lib = _lib.load()
        N, Hin, Win, H, W, OH, OW = _dims(shape)
        image, x, g1, g2, w, b, m = _inputs(shape, exact)
        if gy is not None:
            g1 = gy
        if isinstance(gy2, str):
            gy2 = g2
        alloc = G.GuardedAllocator(cuda).install(monkeypatch)
        try:
            cl = lambda t: alloc.guard(t.contiguous(memory_format=torch.channels_last))
            d_image, d_x, d_g1 = cl(image), cl(x), cl(g1)
            d_g2 = cl(gy2) if gy2 is not None else None
            d_w, d_b, d_m = alloc.guard(w), alloc.guard(b), alloc.guard(m)
            d_v = alloc.guard(torch.full((C,), VAR))
            st = _lib.stream_ptr(cuda)
            P = _lib.ptr
            y = torch.empty((N, C, OH, OW), device=cuda, memory_format=torch.channels_last)
            rec = torch.empty((int(lib.mr_stem_pool_records_bytes(N, C, H, W)),), dtype=torch.uint8, device=cuda)
            _lib.call("mr_stem_pool_forward", P(d_x), P(d_w), P(d_b), P(d_m), P(d_v), EPS, 0, 2, P(y), P(rec), N, C, H, W, st)
            wb = int(lib.mr_stem_pool_backward_workspace_bytes(N, C, H, W))
            gmap = torch.empty((N, C, H, W), device=cuda, memory_format=torch.channels_last)
            bn_gw, bn_gb, work = torch.empty(C, device=cuda), torch.empty(C, device=cuda), torch.empty(wb, dtype=torch.uint8, device=cuda)
            _lib.call("mr_stem_pool_backward", P(d_g1), P(d_g2), None, P(rec), P(d_w), P(d_b), P(d_m), P(d_v), EPS, 0, 2, P(gmap),
                      P(bn_gw), P(bn_gb), P(work), wb, N, C, H, W, st)
            # the new entry points
            s_gw, s_gb, work2 = torch.empty(C, device=cuda), torch.empty(C, device=cuda), torch.empty(wb, dtype=torch.uint8, device=cuda)
            _lib.call("mr_stem_pool_param_grads", P(d_g1), P(d_g2), P(rec), P(d_w), P(d_b), P(d_m), P(d_v), EPS, 0, P(s_gw), P(s_gb),
                      P(work2), wb, N, C, H, W, st)
            wsb = int(lib.mr_stem_conv_wrw_workspace_bytes(N, C, Hin, Win))
            assert wsb > 0
            fmt = torch.channels_last if weight_cl else torch.contiguous_format
            outs = []
            for _ in range(2 if repeat else 1):
                gw = torch.empty((C, 3, 7, 7), device=cuda, memory_format=fmt)
                work3 = torch.empty(wsb, dtype=torch.uint8, device=cuda)
                _lib.call("mr_stem_conv_wrw", P(d_g1), P(d_g2), P(rec), P(d_w), P(d_b), P(d_m), P(d_v), EPS, P(d_image), P(gw),
                          int(weight_cl), P(work3), wsb, N, C, Hin, Win, 3, 7, 2, 3, st)
                outs.append(gw)
            damage = alloc.check()
            assert not damage, "\n".join(damage)
            self.gw = outs[0].cpu().contiguous()
            self.gw_again = outs[-1].cpu().contiguous()
            self.gmap_dev, self.image_dev = gmap.contiguous(memory_format=torch.channels_last), d_image
            self.gmap = gmap.cpu()
            self.bn = (bn_gw.cpu(), bn_gb.cpu())
            self.bn_sums_only = (s_gw.cpu(), s_gb.cpu())
            self.image = image
        finally:
            alloc.uninstall()

    def reference(self):
        """fp64 on the CPU from the map the existing backward wrote"""
        return torch.nn.grad.conv2d_weight(self.image.double(), (C, 3, 7, 7), self.gmap.double().contiguous(), stride=2, padding=3)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, max |diff| {float(d.max()):g}")


@pytest.mark.parametrize("two", [True, False], ids=["two_gradients", "one_gradient"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact(cuda, monkeypatch, shape, two):
    shape = _shape(shape)
    r = Run(cuda, monkeypatch, shape, True, gy2="default" if two else None)
    ref = r.reference()
    assert float(r.gmap.abs().max()) > 0
    assert float(ref.abs().max()) < 2 ** 23  # (in halves: below 2^24, exact in fp32)
    _same(r.gw, ref.float(), f"grad_conv_weight {shape}")
    _same(r.bn_sums_only[0], r.bn[0], "bn grad_weight of the sums-only form")
    _same(r.bn_sums_only[1], r.bn[1], "bn grad_bias of the sums-only form")


def test_exact_contiguous_weight_layout(cuda, monkeypatch):
    r = Run(cuda, monkeypatch, (2, 22, 18), True, weight_cl=False)
    _same(r.gw, r.reference().float(), "grad_conv_weight, [C][ci][kh][kw]")


def test_zero_gradient_gives_exact_zero(cuda, monkeypatch):
    shape = (2, 23, 19)
    N, Hin, Win, H, W, OH, OW = _dims(shape)
    z = torch.zeros(N, C, OH, OW)
    r = Run(cuda, monkeypatch, shape, True, gy=z, gy2=z)
    assert r.gw.shape == (C, 3, 7, 7) and int((r.gw != 0).sum()) == 0 and not bool(torch.signbit(r.gw).any())


@pytest.mark.parametrize("shape", [(2, 23, 19), (3, 36, 70)], ids=str)
def test_gradient_in_the_corner_windows_only(cuda, monkeypatch, shape):
    N, Hin, Win, H, W, OH, OW = _dims(shape)
    g1 = _inputs(shape, True)[2]
    corner = torch.zeros_like(g1)
    for oy in (0, OH - 1):
        for ox in (0, OW - 1):
            corner[:, :, oy, ox] = g1[:, :, oy, ox] + (g1[:, :, oy, ox] == 0).float()  # (non-zero everywhere)
    r = Run(cuda, monkeypatch, shape, True, gy=corner, gy2=None)
    assert float(r.gmap.abs().max()) > 0
    _same(r.gw, r.reference().float(), f"grad_conv_weight, corner windows {shape}")


def test_two_calls_give_the_same_bits(cuda, monkeypatch):
    r = Run(cuda, monkeypatch, (3, 36, 70), False, repeat=True)
    _same(r.gw_again, r.gw, "second call")


@pytest.mark.parametrize("shape", [(3, 36, 70), "tiles"], ids=str)
def test_random_data_against_the_composed_path(cuda, monkeypatch, shape):
    """Figures on an MI355X (printed by this test, kept in profiles/stem_wrw_ab.txt): (3, 36, 70) new kernel 6.1e-8, composed
    path 2.7e-7; the tile-derived shape 7.1e-8 against 4.4e-7 .. 6.0e-7."""
    shape = _shape(shape)
    r = Run(cuda, monkeypatch, shape, False)
    ref = r.reference()
    parent = torch.nn.grad.conv2d_weight(r.image_dev, (C, 3, 7, 7), r.gmap_dev, stride=2, padding=3).cpu()
    scale = float(ref.abs().max())
    err_new = float((r.gw.double() - ref).abs().max()) / scale
    err_parent = float((parent.double() - ref).abs().max()) / scale
    line = f"STEM-WRW random {shape}: max|gW| {scale:.4g}  new kernel {err_new:.3e}  composed path (MIOpen) {err_parent:.3e}"
    print(line)
    assert bool(torch.isfinite(r.gw).all())
    assert err_new <= 2 * err_parent, line
    _same(r.bn_sums_only[0], r.bn[0], "bn grad_weight of the sums-only form")
    _same(r.bn_sums_only[1], r.bn[1], "bn grad_bias of the sums-only form")


def test_argument_checks_launch_nothing(cuda):
    """each refused call returns MR_ERR_BADARG before the first HIP call: the output keeps its poison"""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    N, Hin, Win, H, W, OH, OW = _dims((2, 22, 18))
    P = _lib.ptr
    rec = torch.zeros(int(lib.mr_stem_pool_records_bytes(N, C, H, W)) + 16, dtype=torch.uint8, device=cuda)
    gy = torch.zeros(N * OH * OW * C + 4, device=cuda)
    chan = torch.ones(C, device=cuda)
    image = torch.zeros(N * Hin * Win * 3, device=cuda)
    wsb = int(lib.mr_stem_conv_wrw_workspace_bytes(N, C, Hin, Win))
    work = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    out = torch.full((C * 147,), 7.0, device=cuda)
    assert rec.data_ptr() % 16 == 0 and gy.data_ptr() % 16 == 0

    def call(**over):
        a = dict(gy=P(gy), gy2=None, rec=P(rec), image=P(image), out=P(out), work=P(work), wbytes=wsb, C=C, cin=3, k=7, s=2, p=3)
        a.update(over)
        return lib.mr_stem_conv_wrw(a["gy"], a["gy2"], a["rec"], P(chan), P(chan), P(chan), P(chan), 1e-5, a["image"], a["out"], 1,
                                    a["work"], a["wbytes"], N, a["C"], Hin, Win, a["cin"], a["k"], a["s"], a["p"], _lib.stream_ptr(cuda))

    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    for name, over in [("kernel size", dict(k=5)), ("stride", dict(s=1)), ("padding", dict(p=2)), ("Cin", dict(cin=4)),
                       ("C % 4", dict(C=62)), ("C", dict(C=32)), ("misaligned records", dict(rec=off(rec, 4))),
                       ("misaligned gradient", dict(gy=off(gy, 4))), ("misaligned second gradient", dict(gy2=off(gy, 8))),
                       ("short workspace", dict(wbytes=wsb - 1)), ("no workspace", dict(work=None)), ("no image", dict(image=None)),
                       ("no output", dict(out=None))]:
        assert call(**over) == -1, name
    assert lib.mr_stem_conv_wrw_workspace_bytes(N, 62, Hin, Win) == -1
    assert lib.mr_stem_conv_wrw_workspace_bytes(-1, C, Hin, Win) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert int((out != 0).sum()) == 0  # (zero gradient)
