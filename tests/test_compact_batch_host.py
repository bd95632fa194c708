"""The compact image batch's host side, without a GPU: the MR_DTYPE_* codes and what the entry points answer to codes they
refuse, the new rows of the ctypes table, the dtype gate of the fused pair path (``_lib.batch_dtypes``), the dtype word of the
pair-step struct and the plan key that keeps batches of different types apart, and ``frames_to_batch``'s argument checks."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshraster_hip.h")
F32, BF16, U8 = 0, 1, 2


def test_dtype_codes_match_the_header():
    from handobjectconsist_amd import _lib

    defs = dict(re.findall(r"^#define\s+MR_DTYPE_([A-Z0-9]+)\s+(\d+)\s*$", open(HEADER).read(), re.M))
    assert defs == {"F32": "0", "BF16": "1", "U8": "2"}
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_U8) == (F32, BF16, U8)
    assert _lib.DTYPE_CODES == {torch.float32: F32, torch.bfloat16: BF16, torch.uint8: U8}


def test_typed_rows_extend_the_rows_they_generalise():
    """SIGNATURES lists the three *_typed entry points (tests/test_abi.py checks every row against the header's prototypes):
    each is its untyped form's row plus the two dtype codes, and the library exports it."""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    for typed, base in (("mr_frames_to_batch_typed", "mr_frames_to_batch"),
                        ("mr_flow_pair_forward_tiles_typed", "mr_flow_pair_forward_tiles_crit"),
                        ("mr_flow_pair_forward_grad_tiles_typed", "mr_flow_pair_forward_grad_tiles_crit")):
        res, args = _lib.SIGNATURES[typed]
        bres, bargs = _lib.SIGNATURES[base]
        assert res is bres and args == bargs + [ctypes.c_int, ctypes.c_int], typed
        assert hasattr(lib, typed)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for typed in ("mr_flow_pair_forward_tiles_typed", "mr_flow_pair_forward_grad_tiles_typed"):
        proto = re.search(r"MR_API\s+int\s+" + typed + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        for name in ("image_ref", "image", "jitter_ref", "jitter"):
            assert re.search(r"const\s+void\s*\*\s*" + name + r"\b", proto), (typed, name)


def _frames_typed(lib, image_dtype, mask_dtype, num_frames=2):
    p = ctypes.c_void_p(0x1000)
    return lib.mr_frames_to_batch_typed(p, p, None, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0, p, 1 << 30, p, p, 3, num_frames, 8, 8, 8, 8, None,
                                        image_dtype, mask_dtype)


def test_frame_kernel_refuses_unknown_dtype_codes_before_any_device_work():
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    # (an empty batch returns MR_OK without touching the device: the codes are checked before that)
    for idt, mdt in ((F32, F32), (BF16, U8), (BF16, F32), (F32, U8)):
        assert _frames_typed(lib, idt, mdt, num_frames=0) == 0, (idt, mdt)
    for idt, mdt in ((3, F32), (-1, F32), (U8, F32), (F32, BF16), (BF16, 3), (F32, -1), (256, F32), (BF16, 258)):
        assert _frames_typed(lib, idt, mdt, num_frames=0) == -1, (idt, mdt)
        assert _frames_typed(lib, idt, mdt) == -1, (idt, mdt)


def _flow_fwd_typed(lib, name, image_dtype, mask_dtype, **over):
    """the entry point on test_abi's valid argument set (every pointer non-NULL and never dereferenced; an empty batch
    returns before the first HIP call)"""
    from tests.test_abi import _VALID, _prototype

    args = []
    for kind, p in _prototype(name):
        if kind == "stream":
            args.append(None)
        elif kind == "ptr":
            args.append(over.get(p, 0x1000))
        elif kind == "float":
            args.append(0.5)
        elif p == "image_dtype":
            args.append(image_dtype)
        elif p == "mask_dtype":
            args.append(mask_dtype)
        else:
            args.append(int(over.get(p, _VALID[p])))
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", ["mr_flow_pair_forward_tiles_typed", "mr_flow_pair_forward_grad_tiles_typed"])
def test_flow_pair_forward_accepts_three_dtype_pairs(name):
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    empty = dict(batch_size=0, list_capacity=0)
    for idt, mdt in ((F32, F32), (BF16, U8), (BF16, F32)):
        assert _flow_fwd_typed(lib, name, idt, mdt, **empty) == 0, (idt, mdt)
        assert _flow_fwd_typed(lib, name, idt, mdt, image=None, **empty) == -1  # (the shared checks still run)
        assert _flow_fwd_typed(lib, name, idt, mdt, criterion=2, **empty) == -1
    assert _flow_fwd_typed(lib, name, F32, U8, **empty) == -2, "valid codes without a kernel: MR_ERR_NOTIMPL"
    for idt, mdt in ((3, F32), (U8, U8), (BF16, BF16), (-1, F32), (F32, 7)):
        assert _flow_fwd_typed(lib, name, idt, mdt, **empty) == -1, (idt, mdt)


def test_pair_step_struct_carries_the_dtypes_in_reserved():
    """MrPairStep keeps its size and field list (tests/test_abi.py pins both); the word named ``reserved`` holds the image
    dtype in bits 0-7 and the mask dtype in bits 8-15, zero meaning what it always meant."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    assert "reserved" in [f for f, _ in pairstep.MrPairStep._fields_]
    lib = _lib.load()
    st = pairstep.MrPairStep()
    for k, v in dict(batch_size=2, num_verts_a=778, num_verts_b=1002, num_hand_faces=1552, num_obj_faces=2000, fill_back=1,
                     image_size=64, height=64, width=64, jitter_channels=3).items():
        setattr(st, k, v)
    sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    sizes = {}
    for word, rc in ((0, 0), (BF16 | (U8 << 8), 0), (BF16, 0), (F32 | (U8 << 8), -2), (3, -1), (U8, -1), (BF16 | (BF16 << 8), -1),
                     (BF16 | (U8 << 8) | (1 << 16), -1), (-1, -1)):
        st.reserved = word
        assert lib.mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == rc, word
        if rc == 0:
            sizes[word] = (sc.value, sv.value, th.value)
    assert len(set(sizes.values())) == 1, "the scratch / saved layout does not depend on the batch's element types"


def test_dtype_gate_of_the_fused_pair_path():
    from handobjectconsist_amd import _lib

    f32, bf16, u8 = torch.float32, torch.bfloat16, torch.uint8
    z = lambda dt: torch.zeros(1, dtype=dt)  # noqa: E731
    gate = lambda a, b, c, d: _lib.batch_dtypes(z(a), z(b), z(c), z(d))  # noqa: E731  (image_ref, image, jitter_ref, jitter)
    assert gate(f32, f32, f32, f32) == (f32, f32)
    assert gate(bf16, bf16, u8, u8) == (bf16, u8)
    assert gate(bf16, bf16, f32, f32) == (bf16, f32)
    # fp32 images: masks of any type are read as fp32 (cast by the caller, as ever)
    assert gate(f32, f32, u8, u8) == (f32, f32) and gate(f32, f32, torch.bool, f32) == (f32, f32)
    # both images of one type, both masks of one type; nothing but bf16 / uint8 is compact
    for combo in ((f32, bf16, u8, u8), (bf16, bf16, u8, f32), (bf16, bf16, f32, u8), (bf16, bf16, bf16, bf16),
                  (bf16, bf16, torch.bool, torch.bool), (torch.float16, torch.float16, u8, u8),
                  (torch.float64, torch.float64, f32, f32), (u8, u8, u8, u8)):
        assert gate(*combo) is None, combo
    assert set(_lib.FUSED_BATCH_DTYPES) == {(f32, f32), (bf16, u8), (bf16, f32)}


def test_flow_pair_loss_returns_none_for_unsupported_batches(monkeypatch):
    """The gate in flow_pair_loss: a batch the kernels have no instantiation for falls to the composed path (None) before
    anything is launched, whatever the rest of the configuration says; a supported one gets past the dtype condition (here:
    to the stubbed struct path)."""
    from handobjectconsist_amd.warping import opticalflow, pairstep

    class Ren:
        image_size, anti_aliasing, fill_back = 64, False, True

        def render_projected_vertex_colors(self):
            pass

    class FakeCuda(torch.Tensor):  # (CPU storage that says it is on the device: only the gate is exercised)
        is_cuda = True

    monkeypatch.setattr(opticalflow, "_vertex_color_path", lambda ren, detach: True)
    reached = []
    monkeypatch.setattr(pairstep, "pair_step", lambda *a, **k: reached.append(tuple(x.dtype for x in a[10:14])))
    fake = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype).as_subclass(FakeCuda)  # noqa: E731
    B = 2
    h, o = fake(B, 778, 3).requires_grad_(True), fake(B, 1002, 3)
    faces = (fake(1552, 3, dtype=torch.int64), fake(B, 2000, 3, dtype=torch.int64))
    K = [torch.eye(3).repeat(B, 1, 1)] * 2
    f32, bf16, u8 = torch.float32, torch.bfloat16, torch.uint8

    def run(ir, im, jr, jm):
        del reached[:]
        imgs = [fake(B, 3, 64, 64, dtype=d) for d in (ir, im)] + [fake(B, 3, 64, 64, dtype=d) for d in (jr, jm)]
        try:
            res = opticalflow.flow_pair_loss([(h, o), (h, o)], faces, K, Ren(), (64, 64), *imgs)
        except Exception:  # (past the gate and the stub: the node pair needs a device)
            return "passed the gate"
        return res

    for combo in ((f32, f32, f32, f32), (bf16, bf16, u8, u8), (bf16, bf16, f32, f32)):
        assert run(*combo) == "passed the gate" and reached and reached[0] == combo, combo
    for combo in ((bf16, bf16, u8, f32), (f32, bf16, u8, u8), (torch.float16, torch.float16, u8, u8), (bf16, bf16, bf16, bf16)):
        assert run(*combo) is None and not reached, combo


def test_pair_step_plans_are_not_shared_between_batch_formats(monkeypatch):
    """pair_step keys its plan on the batch's element types and writes them into MrPairStep.reserved; a batch without a
    kernel gives None.  The device call is replaced (no GPU here), as in tests/test_l2_criterion_host.py."""
    from handobjectconsist_amd.warping import pairstep

    seen = []

    def fake_apply(h1, o1, h2, o2, call):
        plan, images = call[0], call[6]
        seen.append((plan, int(plan.st.reserved), tuple(x.dtype for x in images)))
        raise StopIteration

    class Ren:
        R, t, dist_coeffs = torch.eye(3)[None], torch.zeros(1, 3), torch.zeros(1, 5)
        background_color = [0.0, 0.0, 0.0]
        orig_size, near, far, rasterizer_eps, fill_back = 64, 0.1, 100.0, 1e-3, True

    monkeypatch.setattr(pairstep._PairStepFunction, "apply", staticmethod(fake_apply))
    monkeypatch.setattr(pairstep.torch._C, "_cuda_getCurrentRawStream", lambda idx: 0)
    monkeypatch.setattr(pairstep.torch.cuda, "is_current_stream_capturing", lambda: True)  # (no pinned word: no device)
    monkeypatch.setattr(pairstep._Plan, "ensure_scratch", lambda self: None)
    monkeypatch.setattr(pairstep, "_PLANS", {})
    import handobjectconsist_amd.neurender.rasterize as rasterize

    monkeypatch.setattr(rasterize, "_background_tensor", lambda bg, dev, n: (torch.zeros(3), 0))
    B, Va, Vb, H = 2, 778, 1002, 64
    h1, o1 = torch.zeros(B, Va, 3), torch.zeros(B, Vb, 3)
    hf, of = torch.zeros(1552, 3, dtype=torch.int64), torch.zeros(B, 2000, 3, dtype=torch.int64)
    K = torch.eye(3).repeat(B, 1, 1)
    f32, bf16, u8 = torch.float32, torch.bfloat16, torch.uint8

    def step(idt, mdt, idt_ref=None):
        img, jit = torch.zeros(B, 3, H, H, dtype=idt), torch.ones(B, 3, H, H, dtype=mdt)
        ref = img if idt_ref is None else img.to(idt_ref)
        try:
            return pairstep.pair_step((h1, o1), (h1, o1), hf, of, K, K, Ren(), 64, H, H, ref, img, jit, jit, None)
        except StopIteration:
            return "called"

    for idt, mdt in ((f32, f32), (bf16, u8), (bf16, f32), (f32, u8), (bf16, u8)):
        assert step(idt, mdt) == "called"
    words = [w for _, w, _ in seen]
    assert words == [0, BF16 | (U8 << 8), BF16, 0, BF16 | (U8 << 8)]
    assert [d for _, _, d in seen] == [(f32,) * 4, (bf16, bf16, u8, u8), (bf16, bf16, f32, f32), (f32,) * 4, (bf16, bf16, u8, u8)], \
        "a compact batch goes in as it is; fp32 images take fp32 masks"
    plans = [p for p, _, _ in seen]
    assert plans[0] is plans[3] and plans[1] is plans[4] and len({id(p) for p in plans}) == 3
    assert step(bf16, u8, idt_ref=f32) is None and step(torch.float16, u8) is None and step(bf16, torch.bool) is None
    assert len(seen) == 5


def test_frames_to_batch_validates_its_dtype_arguments():
    from handobjectconsist_amd.datasets import frames as F

    frames = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    ident = [[1.0, 0, 0, 0, 1.0, 0]]
    for kw in (dict(image_dtype=torch.float16), dict(image_dtype=torch.uint8), dict(mask_dtype=torch.bfloat16),
               dict(mask_dtype=torch.bool), dict(image_dtype=None), dict(mask_dtype="uint8")):
        with pytest.raises(ValueError, match="dtype"):
            F.frames_to_batch(frames, ident, (4, 4), **kw)
    with pytest.raises(TypeError):  # (valid types: the next check is the device's)
        F.frames_to_batch(frames, ident, (4, 4), image_dtype=torch.bfloat16, mask_dtype=torch.uint8)


def test_encoder_casts_a_bf16_batch_to_the_first_convolutions_type_without_autocast():
    from handobjectconsist_amd.models.synthnet import SynthMeshRegNet

    net = SynthMeshRegNet.__new__(SynthMeshRegNet)
    torch.nn.Module.__init__(net)
    seen = []

    class Trunk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(3, 4, 3)

        def forward(self, x):
            seen.append(x.dtype)
            return x.float().mean((2, 3))

    net.base_net, net.encoder_dtype = Trunk(), torch.float32
    img = torch.zeros(1, 3, 8, 8)
    net.encode(img.bfloat16())
    net.encode(img)
    assert seen == [torch.float32, torch.float32]
