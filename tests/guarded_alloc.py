"""Guard-band allocator for tests (a helper module: no fixtures, nothing pytest collects).

The value tests cannot see a kernel that stores a few elements past the end of an output, a workspace or a gradient
buffer: the caching allocator rounds every block up to 512 bytes, so the overrun lands in padding or in an unrelated live
tensor, nothing faults and no compared value changes.  ``GuardedAllocator`` closes that gap without any tool: while it is
installed, the torch factories below hand out, for tensors on the guarded device, the INTERIOR of a larger uint8 backing
buffer

    [ band of 0xFF | interior (nbytes) | band of 0xFF ]

and ``check()`` afterwards compares every band with the pattern it was filled with.  0xFF bytes are NaN in fp32, bf16 and
fp64 and 255 in u8, so an over-READ that is used shows up in the result as well; the interior of an ``empty*`` tensor is
filled with 0xFF too, so an element nobody writes is a NaN.

The returned tensor is NOT a view: it is built with ``Tensor.set_`` on the backing buffer's untyped storage (offset, size,
strides).  The package reads ``._base`` (``imgflowarp._stacked_base``) and ties hand-overs to ``._version``; a ``narrow`` /
``as_strided`` view would send the guarded run down other code paths than the plain run.  (``set_`` leaves ``_version`` at 1
where a fresh tensor has 0: the package only ever compares the version of one tensor with an earlier reading of the same
tensor.)

The eight factories are not the only way a tensor comes to be: ``cat``, ``to``, ``contiguous``, ``clone``, arithmetic ... allocate
inside torch.  While the allocator is installed a ``TorchDispatchMode`` therefore RE-HOMES every freshly allocated result of
a torch op on the guarded device: it is copied into guarded storage (same dtype, shape and strides) and that tensor is
returned in its place -- below autograd, so graphs, values and layouts are what they would have been.  Views and in-place
results (storage shared with an operand) stay what they are.  Re-homed index tensors (int32 / int64) get bands of zero bytes,
as ``guard()`` gives them.  What the mode does NOT touch: the results of the factory ops themselves (a factory taken out of the
patch list hands out plain memory), anything made under ``paused()`` or before the allocator was installed, and memory torch
did not allocate.  ``pointer_report`` names every such pointer that reaches the C-ABI.

Used with ``monkeypatch`` (``alloc.install(monkeypatch)``) or as a context manager.
"""
import ctypes
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten, tree_map

BAND = 4096  # bytes on either side; a multiple of 256 (the interior keeps the alignment the entry points check: & 15, & 7,
#              & 3) and wider than one 16-byte store per lane of a 256-thread workgroup
ALIGN = 256
PATTERN = 0xFF
assert BAND % ALIGN == 0

FACTORIES = ("empty", "zeros", "full", "ones")
LIKE_FACTORIES = ("empty_like", "zeros_like", "full_like", "ones_like")
_INDEX_DTYPES = (torch.int32, torch.int64)
_THIS_FILE = os.path.abspath(__file__).rstrip("c")
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep


def _site():
    """file:line (function) of the first frame outside this module"""
    f = sys._getframe(1)
    while f is not None and (os.path.abspath(f.f_code.co_filename).rstrip("c") == _THIS_FILE
                             or os.path.abspath(f.f_code.co_filename).startswith(_TORCH_DIR)):
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.relpath(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"


def _span_bytes(size, stride, itemsize):
    """bytes from the first to one past the last element of a (size, stride) layout"""
    if any(s == 0 for s in size):
        return 0
    return (1 + sum((s - 1) * st for s, st in zip(size, stride))) * itemsize


def is_dense(t):
    """non-overlapping and dense: the strides are a permutation of a contiguous layout"""
    if t.numel() == 0:
        return True
    dims = sorted((st, s) for s, st in zip(t.shape, t.stride()) if s != 1)
    expect = 1
    for st, s in dims:
        if st != expect:
            return False
        expect *= s
    return True


class Entry:
    __slots__ = ("backing", "offset", "nbytes", "dtype", "site", "pattern", "kind")

    def __init__(self, backing, offset, nbytes, dtype, site, pattern, kind):
        self.backing, self.offset, self.nbytes, self.dtype = backing, offset, nbytes, dtype
        self.site, self.pattern, self.kind = site, pattern, kind

    @property
    def start(self):
        return self.backing.data_ptr() + self.offset

    def __iter__(self):  # (backing, interior offset, nbytes, dtype, where allocated)
        return iter((self.backing, self.offset, self.nbytes, self.dtype, self.site))


class GuardedAllocator:
    def __init__(self, device, band=BAND, leave_out=()):
        """``leave_out``: names of factories NOT to patch (the self-test of the pointer check: what they allocate must then be
        reported as a stranger)"""
        assert band % ALIGN == 0 and band > 0 and set(leave_out) <= set(FACTORIES + LIKE_FACTORIES)
        self.device = self._norm(torch.device(device))
        self.band = band
        self.registry = []
        self._real = {n: getattr(torch, n) for n in FACTORIES + LIKE_FACTORIES}
        self._patched = {n: self._make(n) for n in FACTORIES + LIKE_FACTORIES if n not in leave_out}
        self._undo = None
        self._busy = 0  # > 0: inside the allocator's own torch calls (the re-homing mode lets them through)
        self._mode = _Rehome(self)
        self._storages = set()  # data pointers of the backing buffers' storages
        self.rehomed = 0

    # ---------------------------------------------------------------- installation
    def install(self, monkeypatch):
        """patch the factories through ``monkeypatch`` and enter the re-homing mode; ``uninstall()`` (or the end of the test,
        for the factories) undoes it"""
        for n, fn in self._patched.items():
            monkeypatch.setattr(torch, n, fn)
        self._mode.__enter__()
        self._monkeypatch = monkeypatch
        return self

    def uninstall(self):
        self._mode.__exit__(None, None, None)
        for n in self._patched:
            self._monkeypatch.setattr(torch, n, self._real[n])

    def paused(self):
        """context manager: torch calls inside it are left alone by the re-homing mode (for tensors a test wants OUTSIDE
        guarded storage; the patched factories still guard)"""
        return _Paused(self)

    def __enter__(self):
        self._undo = {n: getattr(torch, n) for n in self._patched}
        for n, fn in self._patched.items():
            setattr(torch, n, fn)
        self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        self._mode.__exit__(None, None, None)
        for n, fn in self._undo.items():
            setattr(torch, n, fn)
        self._undo = None
        return False

    # ---------------------------------------------------------------- the factories
    @staticmethod
    def _norm(dev):
        if dev.type == "cuda" and dev.index is None:
            return torch.device("cuda", torch.cuda.current_device())
        return dev

    def _guards(self, dev):
        if dev is None:
            dev = torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
        elif isinstance(dev, int):
            dev = torch.device("cuda", dev)
        else:
            dev = torch.device(dev)
        return self._norm(dev) == self.device

    def _make(self, name):
        real = self._real[name]
        like = name.endswith("_like")
        kind = name.split("_")[0]

        def factory(*args, **kw):
            self._busy += 1
            try:
                return guarded(*args, **kw)
            finally:
                self._busy -= 1

        def guarded(*args, **kw):
            if kw.get("out") is not None or kw.get("pin_memory") or kw.get("names") is not None \
                    or kw.get("layout", torch.strided) is not torch.strided:
                return real(*args, **kw)
            if like:
                src = args[0] if args else kw.get("input")
                if not isinstance(src, torch.Tensor) or src.layout is not torch.strided or src.is_sparse:
                    return real(*args, **kw)
                dev = kw.get("device")
                if not self._guards(src.device if dev is None else dev):
                    return real(*args, **kw)
            elif not self._guards(kw.get("device")):
                return real(*args, **kw)
            # torch itself parses the arguments: the meta tensor has the size, strides and dtype the real call would give
            meta = real(*args, **dict(kw, device="meta", requires_grad=False))
            fill = None
            if kind == "zeros":
                fill = 0
            elif kind == "ones":
                fill = 1
            elif kind == "full":
                fill = args[1] if len(args) > 1 else kw["fill_value"]
            t = self._alloc(tuple(meta.shape), tuple(meta.stride()), meta.dtype, fill, _site(), name, PATTERN)
            if kw.get("requires_grad"):
                t.requires_grad_(True)
            return t

        factory.__name__ = "guarded_" + name
        return factory

    def _alloc(self, size, stride, dtype, fill, site, kind, pattern):
        itemsize = self._real["empty"]((), dtype=dtype, device="meta").element_size()
        nbytes = _span_bytes(size, stride, itemsize)
        backing = self._real["empty"]((self.band + nbytes + self.band + ALIGN,), dtype=torch.uint8, device=self.device)
        backing.fill_(pattern)
        offset = self.band + (-(backing.data_ptr() + self.band)) % ALIGN
        if nbytes and pattern != PATTERN:  # (an unwritten interior is 0xFF whatever the bands hold)
            backing[offset:offset + nbytes].fill_(PATTERN)
        storage = backing.untyped_storage()
        self._storages.add(storage.data_ptr())

        def tensor():
            return self._real["empty"]((0,), dtype=dtype, device=self.device).set_(storage, offset // itemsize, size, stride)

        if fill is not None and nbytes:
            if isinstance(fill, (int, float, bool)) and fill == 0:
                backing[offset:offset + nbytes].zero_()
            else:
                tensor().fill_(fill)  # (through an alias: the tensor handed out has seen no in-place op)
        self.registry.append(Entry(backing, offset, nbytes, dtype, site, pattern, kind))
        return tensor()

    def guard(self, t):
        """A copy of a tensor the test made, in guarded storage (same dtype, shape, strides of a dense source, requires_grad;
        a leaf).  Index tensors (int32 / int64: faces) get bands of ZERO bytes, so that an over-read can never become a wild
        address; every other input keeps 0xFF."""
        if t is None:
            return None
        self._busy += 1
        try:
            return self._guard(t, _site())
        finally:
            self._busy -= 1

    def _guard(self, t, site):
        src = t.detach()
        if src.device != self.device:
            src = src.to(self.device)
        stride = tuple(src.stride()) if is_dense(src) else tuple(self._real["empty"](tuple(src.shape), device="meta").stride())
        pattern = 0 if src.dtype in _INDEX_DTYPES else PATTERN
        g = self._alloc(tuple(src.shape), stride, src.dtype, None, site, "guard", pattern)
        if src.numel():
            self._real["empty"]((0,), dtype=src.dtype, device=self.device).set_(
                g.untyped_storage(), g.storage_offset(), tuple(g.shape), tuple(g.stride())).copy_(src)
        if t.requires_grad:
            g.requires_grad_(True)
        return g

    def _rehome(self, out, operands):
        """called by the mode with the result of one torch op"""
        def fresh(o):
            if not isinstance(o, torch.Tensor) or o.layout is not torch.strided or o.device != self.device or o.numel() == 0 \
                    or o.is_meta:
                return False
            p = o.untyped_storage().data_ptr()
            return p not in self._storages and p not in operands

        def move(o):
            if not fresh(o):
                return o
            self.rehomed += 1
            return self._guard(o, site)

        if not any(fresh(o) for o in tree_flatten(out)[0]):
            return out
        site = _site()
        return tree_map(move, out)

    # ---------------------------------------------------------------- the checks
    def check(self):
        """Synchronise, then compare both bands of every allocation with their pattern.  Returns a list of strings, one
        per damaged band: allocation site, side, first and last changed byte offset (relative to the interior: negative =
        before its first byte; after: 0 = the byte right behind its last)."""
        self._busy += 1
        try:
            return self._check()
        finally:
            self._busy -= 1

    def _check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if not self.registry:
            return []
        band = self.band
        rows = []
        for e in self.registry:
            rows.append(e.backing[e.offset - band:e.offset])
            rows.append(e.backing[e.offset + e.nbytes:e.offset + e.nbytes + band])
        pats = torch.tensor([e.pattern for e in self.registry for _ in (0, 1)], dtype=torch.uint8, device=self.device)
        bad = (torch.stack(rows) != pats[:, None]).cpu()
        report = []
        for r in torch.nonzero(bad.any(dim=1)).flatten().tolist():
            e = self.registry[r // 2]
            idx = torch.nonzero(bad[r]).flatten()
            first, last = int(idx[0]), int(idx[-1])
            if r % 2 == 0:
                side, first, last = "before", first - band, last - band
            else:
                side = "after"
            report.append(f"{e.site}: {e.kind} {e.dtype} of {e.nbytes} bytes: band {side} the interior changed, "
                          f"byte offsets {first}..{last} ({int(idx.numel())} bytes)")
        return report

    def regions(self):
        return [(e.start, e.start + e.nbytes) for e in self.registry]

    def count(self):
        return len(self.registry)

    def holds(self, t):
        """does this tensor live inside a guarded interior?"""
        p = t.data_ptr()
        return any(a <= p < b or (p == a == b) for a, b in self.regions())

    def pointer_report(self, calls, constants=()):
        """``calls``: the (name, args) list of a spy on ``_lib.call``; ``constants``: tensors the case declares as read-only
        constants.  Returns (name, argument index or field name, address) of every non-null ``c_void_p`` argument that lies
        neither inside a guarded interior nor inside the storage of a declared constant.  The stream argument is not a
        pointer to data; for ``mr_pair_step_forward`` / ``_backward`` the pointer fields of the MrPairStep block (the first
        argument, or a dict of them a spy has read out) stand in for the arguments."""
        from handobjectconsist_amd import _lib

        import bisect

        interiors = sorted(self.regions())  # (backing buffers are separate allocations: the interiors do not overlap)
        starts = [a for a, _ in interiors]
        consts = [_storage_span(c) for c in constants if c is not None]

        def known(p):
            i = bisect.bisect_right(starts, p) - 1
            if i >= 0 and (p < interiors[i][1] or p == interiors[i][0]):
                return True
            return any(a <= p < b for a, b in consts)

        out = []
        seen = 0
        for name, args in calls:
            if name in ("mr_pair_step_forward", "mr_pair_step_backward"):
                fields = args[0] if isinstance(args[0], dict) else pair_step_pointers(args[0])
                items = list(fields.items())
            else:
                items = [(i, a) for i, a in enumerate(args)
                         if isinstance(a, ctypes.c_void_p) and not isinstance(a, _lib._StreamArg)]
            for key, a in items:
                p = a.value if isinstance(a, ctypes.c_void_p) else a
                if not p:
                    continue
                seen += 1
                if not known(int(p)):
                    out.append((name, key, int(p)))
        self.pointers_seen = seen
        return out


class _Paused:
    def __init__(self, alloc):
        self.alloc = alloc

    def __enter__(self):
        self.alloc._busy += 1

    def __exit__(self, *exc):
        self.alloc._busy -= 1
        return False


# The ops behind the eight patched factories: their results are NOT re-homed.  A factory taken out of the patch list therefore
# hands out plain memory, and ``pointer_report`` names it -- the check that the guard is not vacuous.
_FACTORY_OPS = frozenset("aten::" + n for n in ("empty", "empty_strided", "empty_like", "zeros", "zeros_like", "ones", "ones_like",
                                                "full", "full_like"))
_LIFTS = (torch.ops.aten.lift_fresh.default, torch.ops.aten.lift_fresh_copy.default, torch.ops.aten.lift.default)


class _Rehome(TorchDispatchMode):
    def __init__(self, alloc):
        super().__init__()
        self.alloc = alloc

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        a = self.alloc
        if a._busy or func._schema.name in _FACTORY_OPS:
            return out
        a._busy += 1
        try:
            # (``torch.tensor(data, device=...)`` builds its result with the modes switched off and shows it to them through
            # ``lift_fresh``, which returns its operand: that operand IS the fresh allocation)
            operands = set() if func in _LIFTS else {
                x.untyped_storage().data_ptr() for x in tree_flatten((args, kwargs))[0]
                if isinstance(x, torch.Tensor) and x.layout is torch.strided and not x.is_meta}
            return a._rehome(out, operands)
        finally:
            a._busy -= 1


def _storage_span(t):
    s = t.untyped_storage()
    return (s.data_ptr(), s.data_ptr() + s.nbytes())


def pair_step_pointers(block):
    """{field: address} of the non-null pointer fields of an MrPairStep block (a ``c_void_p`` holding its address)"""
    from handobjectconsist_amd.warping import pairstep

    addr = block.value if isinstance(block, ctypes.c_void_p) else int(block)
    st = pairstep.MrPairStep.from_address(addr)
    out = {}
    for n, ty in pairstep.MrPairStep._fields_:
        if ty is ctypes.c_void_p:
            v = getattr(st, n)
            if v:
                out[n] = int(v)
    return out
