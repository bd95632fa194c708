"""tests/guarded_alloc.py with the CPU as the guarded device: the planted writes are torch writes into a backing buffer the
test owns (inside the allocation, so harmless), and every one has to be reported with its side and offset."""
import ctypes

import pytest
import torch

from tests import guarded_alloc as G


@pytest.fixture
def alloc(monkeypatch):
    a = G.GuardedAllocator("cpu").install(monkeypatch)
    yield a
    a.uninstall()


def test_band_is_a_multiple_of_the_checked_alignments():
    assert G.BAND == 4096 and G.BAND % 256 == 0 and G.BAND > 16 * 256 - 1


def test_untouched_run_reports_nothing(alloc):
    a = torch.empty((3, 5), dtype=torch.float32)
    b = torch.zeros(7, dtype=torch.bfloat16)
    c = torch.full((2, 2), 3.5)
    d = torch.ones(4, dtype=torch.uint8)
    a.fill_(1.0)  # writes inside the interior are no finding
    b += 1
    assert alloc.count() == 4 and alloc.check() == []
    assert torch.equal(c, torch.tensor([[3.5, 3.5], [3.5, 3.5]])) and torch.equal(d, torch.tensor([1, 1, 1, 1], dtype=torch.uint8))
    assert torch.equal(b, torch.ones(7, dtype=torch.bfloat16))


def test_unwritten_empty_interior_is_nan_and_zeros_is_zero(alloc):
    for dt in (torch.float32, torch.bfloat16, torch.float64):
        assert torch.isnan(torch.empty(9, dtype=dt)).all()
        assert torch.isnan(torch.empty_like(torch.zeros(9, dtype=dt))).all()
    assert (torch.empty(9, dtype=torch.uint8) == 255).all()
    assert (torch.zeros(9) == 0).all() and (torch.zeros_like(torch.empty(5)) == 0).all()
    assert (torch.ones_like(torch.empty(5)) == 1).all() and (torch.full_like(torch.empty(5), 2.0) == 2).all()


@pytest.mark.parametrize("where,side,offset", [("just_before", "before", -1), ("just_after", "after", 0),
                                               ("far_before", "before", -G.BAND), ("far_after", "after", G.BAND - 1)])
def test_planted_write_is_reported_with_side_and_offset(alloc, where, side, offset):
    quiet = torch.empty(11, dtype=torch.float32)  # noqa: F841  (a second allocation that stays clean)
    t = torch.empty((5, 3), dtype=torch.float32)
    backing, off, nbytes, dtype, site = alloc.registry[-1]
    assert nbytes == 60 and dtype == torch.float32 and "test_guarded_alloc_host.py" in site
    pos = off + offset if side == "before" else off + nbytes + offset
    backing[pos] = 0
    rep = alloc.check()
    assert len(rep) == 1, rep
    assert "test_guarded_alloc_host.py" in rep[0] and f"band {side} the interior" in rep[0]
    assert f"byte offsets {offset}..{offset} (1 bytes)" in rep[0]
    assert torch.isnan(t).all()  # the interior itself is untouched


def test_first_and_last_changed_offset_of_a_longer_overrun(alloc):
    torch.empty(4, dtype=torch.uint8)
    backing, off, nbytes, _, _ = alloc.registry[-1]
    backing[off + nbytes:off + nbytes + 16] = 7  # one 16-byte store past the end
    backing[off + nbytes + 40] = 7
    rep = alloc.check()
    assert len(rep) == 1 and "after" in rep[0] and "byte offsets 0..40 (17 bytes)" in rep[0]


def test_guarded_tensors_are_no_views_and_keep_dtype_shape_strides_alignment(alloc):
    cases = [torch.empty((2, 3, 5), dtype=torch.float32), torch.empty(2, 3, dtype=torch.bfloat16),
             torch.zeros((7,), dtype=torch.int32), torch.full((3, 1), 2, dtype=torch.int64), torch.ones(1, dtype=torch.float64),
             torch.empty((2, 8, 3, 5), dtype=torch.bfloat16, memory_format=torch.channels_last),
             torch.empty(torch.Size([4, 2]), dtype=torch.uint8), torch.empty((), dtype=torch.float32)]
    want = [((2, 3, 5), (15, 5, 1), torch.float32), ((2, 3), (3, 1), torch.bfloat16), ((7,), (1,), torch.int32),
            ((3, 1), (1, 1), torch.int64), ((1,), (1,), torch.float64), ((2, 8, 3, 5), (120, 1, 40, 8), torch.bfloat16),
            ((4, 2), (2, 1), torch.uint8), ((), (), torch.float32)]
    for t, (shape, stride, dtype) in zip(cases, want):
        assert t._base is None and not t.requires_grad and t.is_leaf
        assert tuple(t.shape) == shape and tuple(t.stride()) == stride and t.dtype == dtype
        assert t.data_ptr() % 256 == 0 and alloc.holds(t)
    assert torch.full((2,), 3).dtype == torch.int64 and torch.full((2,), 1.5).dtype == torch.float32
    assert torch.empty(3, requires_grad=True).requires_grad
    src = torch.randn(2, 8, 3, 5).to(memory_format=torch.channels_last)
    for like in (torch.empty_like(src), torch.zeros_like(src), torch.ones_like(src), torch.full_like(src, 2.0)):
        assert like.stride() == src.stride() and like.is_contiguous(memory_format=torch.channels_last) and like._base is None
    assert torch.empty_like(src, dtype=torch.bfloat16).dtype == torch.bfloat16
    assert torch.empty_like(src, memory_format=torch.contiguous_format).is_contiguous()
    perm = torch.randn(3, 4, 5).permute(2, 0, 1)  # dense, permuted: the strides are kept
    assert torch.empty_like(perm).stride() == perm.stride()
    assert torch.empty_like(torch.randn(6, 6)[:, ::2]).is_contiguous()  # not dense: what torch gives, a dense layout
    assert alloc.check() == []


def test_pass_through_cases_are_passed_through(alloc):
    n = alloc.count()
    out = torch.zeros(4)
    n += 1
    assert alloc.count() == n
    base_ptr = out.data_ptr()
    torch.zeros(4, out=out)
    torch.empty(3, device="meta")
    torch.empty_like(torch.empty(3, device="meta"))
    torch.empty_like(out, device="meta")
    assert alloc.count() == n and out.data_ptr() == base_ptr
    other = G.GuardedAllocator("meta")  # another guarded device: the CPU passes through untouched
    with other:
        t = torch.empty(5)
        assert other.count() == 0 and t.device.type == "cpu"
    assert torch.empty is alloc._patched["empty"]  # the context manager restored what it found
    del t


def test_guard_copies_inputs_and_gives_index_tensors_zero_bands(alloc):
    with alloc:  # (nesting the context manager inside install() is harmless)
        pass
    real_randn = torch.randn(2, 8, 3, 5).to(memory_format=torch.channels_last).requires_grad_(True)
    g = alloc.guard(real_randn)
    assert torch.equal(g, real_randn) and g.stride() == real_randn.stride() and g.requires_grad and g.is_leaf and g._base is None
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    gf = alloc.guard(faces)
    backing, off, nbytes, _, _ = alloc.registry[-1]
    assert torch.equal(gf, faces) and (backing[:off] == 0).all() and (backing[off + nbytes:] == 0).all()
    gs = alloc.guard(torch.arange(12.0).view(3, 4)[:, ::2])  # not dense: a dense copy
    assert gs.is_contiguous() and torch.equal(gs, torch.arange(12.0).view(3, 4)[:, ::2])
    assert alloc.guard(None) is None and alloc.check() == []
    backing[off - 1] = 9  # a zero band reports damage like any other
    rep = alloc.check()
    assert len(rep) == 1 and "before" in rep[0] and "byte offsets -1..-1" in rep[0]


def test_pointer_report_flags_strangers_and_accepts_declared_constants(alloc):
    from handobjectconsist_amd import _lib

    real_empty = alloc._real["empty"]
    inside = torch.empty(16, dtype=torch.float32)
    with alloc.paused():
        const = real_empty(8, dtype=torch.float32)
        stranger = real_empty(8, dtype=torch.float32)
    stream = _lib._StreamArg(0x1234)
    calls = [("mr_some_entry", (_lib.ptr(inside), ctypes.c_void_p(inside.data_ptr() + 60), _lib.ptr(const[2:]), None,
                                ctypes.c_void_p(None), 7, 1.5, stream)),
             ("mr_other_entry", (_lib.ptr(stranger), ctypes.c_void_p(inside.data_ptr() + 64), stream))]
    rep = alloc.pointer_report(calls, constants=[const])
    assert rep == [("mr_other_entry", 0, stranger.data_ptr()), ("mr_other_entry", 1, inside.data_ptr() + 64)]
    assert alloc.pointers_seen == 5
    assert [r[:2] for r in alloc.pointer_report(calls)] == [("mr_some_entry", 2), ("mr_other_entry", 0), ("mr_other_entry", 1)]


def test_pointer_report_reads_the_pair_step_block(alloc):
    from handobjectconsist_amd.warping import pairstep

    inside = torch.empty(16, dtype=torch.float32)
    with alloc.paused():
        stranger = alloc._real["empty"](8, dtype=torch.float32)
    st = pairstep.MrPairStep()
    st.verts1a, st.flows, st.grad_verts1a = inside.data_ptr(), inside.data_ptr() + 4, stranger.data_ptr()
    block = ctypes.c_void_p(ctypes.addressof(st))
    rep = alloc.pointer_report([("mr_pair_step_backward", (block, ctypes.c_void_p(0x99)))])
    assert rep == [("mr_pair_step_backward", "grad_verts1a", stranger.data_ptr())] and alloc.pointers_seen == 3
    snap = G.pair_step_pointers(block)  # a spy reads the block out at call time: the dict stands in for it
    assert alloc.pointer_report([("mr_pair_step_forward", (snap, None))]) == [("mr_pair_step_forward", "grad_verts1a", stranger.data_ptr())]


def test_results_of_torch_ops_are_rehomed_below_autograd(alloc):
    """what ``cat`` / ``to`` / ``contiguous`` / ``clone`` / arithmetic allocate inside torch ends up in guarded storage too: same
    values, dtype, shape and strides, autograd unchanged; views and in-place results stay what they are"""
    with alloc.paused():
        a = alloc._real["empty"](2, 8, 3, 5).normal_().contiguous(memory_format=torch.channels_last)
        idx = torch.tensor([[0, 1, 2]], dtype=torch.int32)
        w = torch.arange(6.0).view(2, 3).clone().requires_grad_(True)
    assert not alloc.holds(a) and not alloc.holds(idx) and not alloc.holds(w)
    n = alloc.count()
    for made in (a.clone(), a * 2, a.to(torch.bfloat16), a.contiguous(), torch.cat([a, a], 0), a + a):
        assert alloc.holds(made) and made._base is None and made.data_ptr() % 256 == 0
    assert alloc.count() == n + 6 == n + alloc.rehomed
    assert torch.equal(a.clone(), a) and a.clone().stride() == a.stride() and a.contiguous().is_contiguous()
    assert a.contiguous(memory_format=torch.channels_last) is a and not alloc.holds(a[1:]) and not alloc.holds(a.mul_(1.0))
    made = torch.tensor([0.1, 0.2, 0.3])  # (built with the modes off, shown to them through lift_fresh)
    assert alloc.holds(made) and made.tolist() == torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64).float().tolist()
    assert alloc.holds(torch.as_tensor([1, 2]).float()) and alloc.holds(torch.arange(4)) and alloc.holds(torch.eye(3)[None])
    both = torch.cat([idx, idx + 3], 0)
    backing, off, nbytes, dtype, _ = alloc.registry[-1]
    assert alloc.holds(both) and dtype == torch.int32 and (backing[:off] == 0).all() and (backing[off + nbytes:] == 0).all()
    assert both.tolist() == [[0, 1, 2], [3, 4, 5]]
    y = (w * 3).t().contiguous()
    assert alloc.holds(y) and y.requires_grad
    y.backward(torch.ones(3, 2))
    assert alloc.holds(w.grad) and torch.equal(w.grad, torch.full((2, 3), 3.0))
    assert alloc.check() == []
    with alloc.paused():
        assert not alloc.holds(a.clone()) and alloc.holds(torch.empty(3))  # paused: the factories still guard


@pytest.mark.parametrize("left_out", G.FACTORIES + G.LIKE_FACTORIES)
def test_a_factory_left_out_of_the_patch_list_hands_out_plain_memory_and_is_reported(monkeypatch, left_out):
    """the check that the guard is not vacuous: the re-homing mode does not pick up what a factory op allocates, so without
    its patch the factory's tensor is a stranger to ``pointer_report``; the other seven still guard"""
    from handobjectconsist_amd import _lib

    a = G.GuardedAllocator("cpu", leave_out=(left_out,)).install(monkeypatch)
    try:
        src = torch.empty(4) if left_out != "empty" else torch.zeros(4)
        assert a.holds(src)
        make = {"empty": lambda: torch.empty(5), "zeros": lambda: torch.zeros(5), "full": lambda: torch.full((5,), 2.0),
                "ones": lambda: torch.ones(5), "empty_like": lambda: torch.empty_like(src), "zeros_like": lambda: torch.zeros_like(src),
                "full_like": lambda: torch.full_like(src, 2.0), "ones_like": lambda: torch.ones_like(src)}
        made = {n: f() for n, f in make.items()}
        assert [n for n, t in made.items() if not a.holds(t)] == [left_out]
        calls = [("mr_entry", tuple(_lib.ptr(t) for t in made.values()))]
        assert a.pointer_report(calls) == [("mr_entry", list(made).index(left_out), made[left_out].data_ptr())]
        assert a.holds(made[left_out].clone())  # what torch derives from it is re-homed as ever
    finally:
        a.uninstall()
    assert torch.empty is a._real["empty"]


def test_an_input_left_out_of_guard_is_reported(alloc):
    """inputs are made outside guarded storage (before the allocator is installed, or under ``paused()``): only ``guard()``
    brings them in"""
    from handobjectconsist_amd import _lib

    with alloc.paused():
        x = alloc._real["empty"](6).normal_().clone()
        idx = torch.tensor([3, 1, 2])
    gx = alloc.guard(x)
    assert not alloc.holds(x) and not alloc.holds(idx) and alloc.holds(gx) and torch.equal(gx, x)
    rep = alloc.pointer_report([("mr_entry", (_lib.ptr(gx), _lib.ptr(idx), _lib.ptr(x)))])
    assert rep == [("mr_entry", 1, idx.data_ptr()), ("mr_entry", 2, x.data_ptr())]
    assert alloc.pointer_report([("mr_entry", (_lib.ptr(gx), _lib.ptr(idx)))], constants=[idx]) == []
