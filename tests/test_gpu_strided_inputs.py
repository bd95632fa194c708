"""Operands that are not freshly made contiguous tensors.  ``_lib.ptr()`` hands ``data_ptr()`` to the C-ABI, so every wrapper
has to make its operands dense first (``_lib.contig``, ``_layout``, ``_aligned``); nothing else in the suite feeds the 19
``torch.autograd.Function``s and the data-path entry points anything but contiguous tensors.

Every case of tests/test_gpu_guard_bands.py that goes through a Python caller runs here with EVERY test-made operand (the
gradients of the backward pass included) turned into a view that holds the same values:

* a step-2 slice of a larger tensor (the innermost dimension of an odd number of elements: rows that start off a 16-byte
  boundary),
* a permuted-back transpose of the two innermost dimensions,
* an offset slice of a larger batch (dense, but the storage starts one row into an allocation); a channels-last activation
  keeps its layout and starts one ELEMENT into a flat buffer, so that no 4-element access of it is aligned -- what
  ``_aligned`` is for,
* the batch-1 camera (K, R, t, dist_coeffs) ``expand``ed to the batch (stride 0),

in rotation, so that neighbouring operands of one call differ in kind (the two drives of the backward start the rotation at
different kinds: every operand is seen in two of them); channels-last operands where the NCHW kernel is the
default and the reverse come with the cases themselves.  The reference run gets ``.contiguous()`` copies of the same views
(``clone(memory_format=torch.preserve_format)`` where the view is dense, so that the same kernel runs).  The backward is
driven once by a gradient made the same way ("sliced") and once by ``sum().backward()`` ("sum": an expanded stride-0
gradient, against ``ones_like``).  Results and leaf gradients are equal bit for bit; the two float-atomics accumulations
keep the tolerance of their parity tests (see test_gpu_guard_bands.py).  What may not happen is a silent different answer."""
import numpy as np
import pytest
import torch

from tests import test_gpu_guard_bands as GB
from tests.guarded_alloc import is_dense

pytestmark = pytest.mark.gpu

# raw entry points on buffers the case allocates itself: no wrapper between the operands and the C-ABI
RAW = ("stem_pool-layout1-",)
NO_BACKWARD = ("occlusion_mask-", "stack_pair_faces-", "hand_verts_batch", "frames_to_batch-", "color_augment-", "jpeg_reconstruct-",
               "png_unfilter-")
KINDS = ("step2", "transpose", "offset")


def as_view(x, kind):
    """a view with the values of ``x`` that is no plain contiguous tensor (``kind``: see the module docstring)"""
    if x.dim() == 0 or x.numel() == 0:
        return x
    if kind == "transpose" and x.dim() < 2:
        kind = "step2"
    if kind == "step2":
        big = torch.zeros(x.shape[:-1] + (2 * x.shape[-1] + 1,), dtype=x.dtype, device=x.device)
        if big.is_floating_point():
            big.fill_(float("nan"))
        view = big[..., 1::2]
        view.copy_(x)
    elif kind == "transpose":
        view = x.transpose(-1, -2).contiguous().transpose(-1, -2)
        if view.is_contiguous():  # (a dimension of one element: nothing to permute)
            return as_view(x, "step2")
    elif x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        # channels-last stays channels-last, one ELEMENT into a flat buffer: no 4-element access of it is aligned
        N, C, H, W = x.shape
        flat = torch.zeros((x.numel() + 2,), dtype=x.dtype, device=x.device)
        if flat.is_floating_point():
            flat.fill_(float("nan"))
        view = flat[1:-1].view(N, H, W, C).permute(0, 3, 1, 2)
        view.copy_(x)
        assert view.is_contiguous(memory_format=torch.channels_last) and view.data_ptr() % (4 * x.element_size())
    else:
        big = torch.zeros((x.shape[0] + 2,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        if big.is_floating_point():
            big.fill_(float("nan"))
        view = big[1:-1]
        view.copy_(x)
    assert torch.equal(view, x) or (x.is_floating_point() and bool(torch.isnan(x).any()))
    return view


def dense_copy(view):
    return view.clone(memory_format=torch.preserve_format) if is_dense(view) else view.contiguous()


class StridedCtx(GB.Ctx):
    """``ctx(x)``: the operand as a view (``copies=False``) or as the contiguous copy of that view (``copies=True``)"""

    def __init__(self, dev, monkeypatch, copies, drive):
        super().__init__(dev, None, monkeypatch)
        self.copies, self.drive, self.n, self.kinds_used = copies, drive, 2 if drive == "sum" else 0, []

    def _view(self, x, kind=None):
        kind = kind or KINDS[self.n % len(KINDS)]
        self.n += 1
        self.kinds_used.append(kind)
        return as_view(x, kind)

    def camera(self, x, B):
        view = x.detach().to(self.dev).expand(B, *x.shape[1:])
        self.kinds_used.append("expand")
        return view.contiguous() if self.copies else view

    def __call__(self, a, grad=False, kind=None):
        if a is None:
            return None
        x = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        view = self._view(x.detach().to(self.dev), kind)
        if self.copies:
            view = dense_copy(view)
        view = view.detach()
        return view.requires_grad_(True) if grad else view

    def backward(self, outs, grads):
        if self.drive == "sum":  # (every output gets an expanded stride-0 gradient of ones)
            if self.copies:
                torch.autograd.backward(list(outs), [torch.ones_like(o) for o in outs])
            else:
                sum(o.sum() for o in outs).backward()
        else:
            torch.autograd.backward(list(outs), list(grads))

    def host(self, a):
        a = np.asarray(a)
        big = np.zeros(a.shape[:-1] + (2 * a.shape[-1] + 1,), a.dtype)
        big[..., 1::2] = a
        view = big[..., 1::2]
        assert not view.flags["C_CONTIGUOUS"] or a.shape[-1] <= 1
        self.kinds_used.append("host-step2")
        return np.ascontiguousarray(view) if self.copies else view


def _names():
    for name in GB.CASES:
        if name.startswith(RAW):
            continue
        yield name, "sliced"
        if not name.startswith(NO_BACKWARD):
            yield name, "sum"


@pytest.mark.parametrize("name,drive", list(_names()))
def test_strided_operands_give_the_answer_of_their_contiguous_copies(cuda, monkeypatch, name, drive):
    from handobjectconsist_amd import _lib

    fn, args, kw = GB.CASES[name]
    reached = set()
    real_call, lib = _lib.call, _lib.load()
    monkeypatch.setattr(_lib, "call", lambda n, *a: (reached.add(n), real_call(n, *a))[1])
    for entry in ("mr_pair_step_forward", "mr_pair_step_backward"):
        monkeypatch.setattr(lib, entry, lambda *a, _real=getattr(lib, entry), _entry=entry: (reached.add(_entry), _real(*a))[1])
    GB._clear_caches()
    ref_ctx = StridedCtx(cuda, monkeypatch, True, drive)
    ref = fn(ref_ctx, *args, **kw)
    GB._clear_caches()
    got_ctx = StridedCtx(cuda, monkeypatch, False, drive)
    got = fn(got_ctx, *args, **kw)
    torch.cuda.synchronize()
    GB._clear_caches()
    assert got_ctx.kinds_used == ref_ctx.kinds_used and got_ctx.kinds_used
    print(f"STRIDED {name} {drive}: operand views {got_ctx.kinds_used}")
    missing = set(got.get("wants_call", ())) - reached
    assert not missing, f"the case did not reach {sorted(missing)}: {sorted(reached)}"
    assert set(got["out"]) == set(ref["out"])
    for key, g in got["out"].items():
        r = ref["out"][key]
        assert (g is None) == (r is None), f"{key}: present in one run only"
        if g is None:
            continue
        g, r = g.detach(), r.detach()
        assert g.shape == r.shape and g.dtype == r.dtype, f"{key}: {tuple(g.shape)} {g.dtype} vs {tuple(r.shape)} {r.dtype}"
        GB._compare(key, g.contiguous(), r.contiguous(), got.get("loose", {}).get(key))
