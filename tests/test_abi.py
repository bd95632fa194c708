"""The C-ABI shared library: loads without a GPU, exports every MR_API prototype of
include/meshraster_hip.h, the ctypes table covers all of them, argument validation happens
before any device work, and the product fails loudly when the library is missing."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshraster_hip.h")


def header_symbols():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"MR_API\s+(?:int64_t|int)\s+(mr_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_five_upstream_entry_points():
    syms = header_symbols()
    for name in ("mr_forward_face_index_map", "mr_forward_texture_sampling", "mr_backward_pixel_map",
                 "mr_backward_textures", "mr_backward_depth_map"):
        assert name in syms
    assert len(syms) >= 15


def test_library_exports_every_declared_symbol():
    from handobjectconsist_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_symbols():
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert sorted(_lib.SIGNATURES) == header_symbols(), "ctypes table and header disagree"
    assert _lib.load().mr_abi_version() == _lib.ABI_VERSION


def test_header_prototype_arity_matches_ctypes_table():
    from handobjectconsist_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        m = re.search(r"MR_API\s+(?:int64_t|int)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), f"{name}: header has {len(params)} parameters, ctypes {len(argtypes)}"


def test_header_prototype_types_match_ctypes_table():
    """... and position by position the KIND of every parameter: pointer / int / int64 / float (a swapped int and float
    would pass the arity check and reinterpret bits at run time), plus the return type."""
    from handobjectconsist_amd import _lib

    def kind(decl):
        decl = decl.strip()
        if "*" in decl or re.search(r"\bmr_stream_t\b", decl):
            return ctypes.c_void_p
        words = decl.split()
        base = [w for w in words[:-1] if w not in ("const", "unsigned")] or words  # (last word = the parameter's name)
        t = base[0]
        return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[t]

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        m = re.search(r"MR_API\s+(int64_t|int)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert res is {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[m.group(1)], f"{name}: return type"
        params = [p for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        for i, (decl, want) in enumerate(zip(params, argtypes)):
            assert kind(decl) is want, f"{name}: parameter {i} `{' '.join(decl.split())}` is bound as {want.__name__}"


def test_pair_step_struct_layout_matches_the_binding():
    """ABI 8: the one argument block of mr_pair_step_* as the library lays it out (size, offset of every field in declaration
    order) against the ctypes Structure of warping/pairstep.py and against the header's field list; sizes need no device."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    lib = _lib.load()
    assert ctypes.sizeof(pairstep.MrPairStep) == lib.mr_pair_step_struct_bytes()
    fields = [f for f, _ in pairstep.MrPairStep._fields_]
    offs = (ctypes.c_int64 * 128)()
    assert lib.mr_pair_step_field_offsets(offs, 128) == len(fields)
    assert [getattr(pairstep.MrPairStep, f).offset for f in fields] == list(offs[:len(fields)])
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct MrPairStep \{(.*?)\} MrPairStep;", src, flags=re.S).group(1)
    decl_names = re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|;)", body)
    assert decl_names == fields, "header and binding list the fields in different orders"
    st = pairstep.MrPairStep()
    for k, v in dict(batch_size=64, num_verts_a=778, num_verts_b=1002, num_hand_faces=1552, num_obj_faces=2000, fill_back=1,
                     image_size=256, height=256, width=256, jitter_channels=3).items():
        setattr(st, k, v)
    sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == 0
    px = 128 * 256 * 256
    assert sv.value >= px * (4 + 12 + 12 + 8) and sc.value >= px * 4 * 6 and th.value == px * 4
    # (every raster the fused path takes: sizes only, whatever the planes' sizes are modulo the regions' 256-byte alignment --
    # a region aliased onto two others refused 36 x 36 and friends for an hour of round 6, found by tests/test_gpu_fuzz.py)
    for B, is_, h, w in ((1, 12, 12, 12), (3, 36, 36, 20), (2, 100, 64, 100), (5, 132, 132, 132), (8, 480, 270, 480), (1, 4, 4, 4)):
        st.batch_size, st.image_size, st.height, st.width = B, is_, h, w
        assert lib.mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == 0, (B, is_)
        assert sc.value >= 2 * B * is_ * is_ * (4 * 6 + 16) and 0 <= th.value - 2 * B * is_ * is_ * 4 < 256 and th.value % 256 == 0
    st.batch_size = 64
    st.image_size = 258  # (not a multiple of 4: the fused path does not apply)
    st.height = st.width = 258
    assert lib.mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == -2
    assert lib.mr_pair_step_forward(None, None) == -1 and lib.mr_pair_step_backward(None, None) == -1


def _header_int(expr):
    """value of a #define's integer expression: literals, parentheses, <<, | and unary minus"""
    import ast

    def ev(n):
        if isinstance(n, ast.Constant) and isinstance(n.value, int):
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        if isinstance(n, ast.BinOp) and isinstance(n.op, (ast.LShift, ast.BitOr)):
            a, b = ev(n.left), ev(n.right)
            return a << b if isinstance(n.op, ast.LShift) else a | b
        raise ValueError(f"unsupported constant expression: {expr}")

    return ev(ast.parse(expr.strip(), mode="eval").body)


def test_header_constants_match_their_python_mirrors():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    src = open(HEADER).read()
    defs = re.findall(r"^#define\s+MR_(FLAG|PAIR_STEP|CRITERION)_([A-Z0-9_]+)\s+(.+?)\s*$", src, re.M)
    kinds = {k for k, _, _ in defs}
    assert kinds == {"FLAG", "PAIR_STEP", "CRITERION"}, kinds
    for kind, name, expr in defs:
        value = _header_int(expr)
        mirror = (pairstep, name) if kind == "PAIR_STEP" else (_lib, f"{kind}_{name}")
        assert hasattr(*mirror), f"MR_{kind}_{name} has no Python mirror ({mirror[0].__name__}.{mirror[1]})"
        assert getattr(*mirror) == value, f"MR_{kind}_{name} = {value}, {mirror[0].__name__}.{mirror[1]} = {getattr(*mirror)}"


def test_argument_validation_needs_no_device():
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    assert lib.mr_render_workspace_bytes(-1, 10, 64) == -1
    assert lib.mr_render_workspace_bytes(2, 100, 64) >= 2 * 100 * (16 + 48)
    assert lib.mr_pair_consist_workspace_bytes(4, 256, 256) == 4 * 4 * 64 * 16
    assert lib.mr_pair_consist_workspace_bytes(1, 0, 5) == -1
    # raster backward scratch (round 3): flags + counts + owner list + per-image owner records, 37 bytes per face and
    # 20 per image up to the 256-byte alignment of its parts; independent of the raster size (no packed map copies)
    w = lib.mr_render_backward_list_workspace_bytes(64, 3076)
    assert 37 * 64 * 3076 <= w <= 37 * 64 * 3076 + 20 * 64 + 5 * 256
    # ... + kernel D's strip bookkeeping (round 4): a weight per (image, axis, strip of 4 lines at 256 x 256) and the
    # per-XCD lists of the strips with work, 4 bytes each
    full = lib.mr_render_backward_workspace_bytes(64, 3076, 256)
    assert w + 2 * 64 * 128 * 4 <= full <= w + 2 * 64 * 128 * 4 + 3 * 256
    assert lib.mr_render_backward_workspace_bytes(-1, 1, 8) == -1
    # trunk glue kernels: 4 bytes x sums per channel (2; bn_add_bn_act 3) x channels x partial-sum slots, + 16.  Slots: the
    # channels-last workgroup cap (2048; stem 4096) or, where larger, the NCHW count -- bn_split = min(ceil(4096 / C), N)
    # sample ranges (1024 at C = 4: the cap holds; 4096 at C = 1: above it), the stem's (sample, 32 x 16 tile) pairs
    # (300 x 5 x 9 = 13500 > 4096).  The launchers take their slot count from the same function, so these numbers also pin
    # the grids of the backward kernels.
    assert lib.mr_bn_act_backward_workspace_bytes(192, 64) == 1048592
    assert lib.mr_bn_act_backward_workspace_bytes(8192, 4) == 2 * 4 * 2048 * 4 + 16 == 65552
    assert lib.mr_bn_act_backward_workspace_bytes(8192, 1) == 2 * 1 * 4096 * 4 + 16
    assert lib.mr_bn_add_bn_act_backward_workspace_bytes(192, 64) == 1572880
    assert lib.mr_stem_pool_backward_workspace_bytes(192, 64, 128, 128) == 2097168
    assert lib.mr_stem_pool_backward_workspace_bytes(300, 4, 257, 257) == 2 * 4 * 13500 * 4 + 16 == 432016
    assert lib.mr_stem_pool_records_bytes(192, 64, 128, 128) == 251658240
    for bad in ((-1, 64), (192, -1)):
        assert lib.mr_bn_act_backward_workspace_bytes(*bad) == -1
        assert lib.mr_bn_add_bn_act_backward_workspace_bytes(*bad) == -1
    for bad in ((-1, 64, 128, 128), (192, -1, 128, 128), (192, 64, -1, 128), (192, 64, 128, -1)):
        assert lib.mr_stem_pool_backward_workspace_bytes(*bad) == -1
        assert lib.mr_stem_pool_records_bytes(*bad) == -1
    assert lib.mr_stem_pool_records_bytes(192, 6, 128, 128) == -1
    null = ctypes.c_void_p(None)
    # NULL pointers / bad sizes are rejected with MR_ERR_BADARG before anything touches HIP
    assert lib.mr_warp_forward(null, null, null, null, 1, 3, 8, 8, 0.99999, 0, null) == -1
    assert lib.mr_backward_textures(null, null, null, null, null, 1, 1, 8, 2, null) == -1
    assert lib.mr_face_inv_map(null, null, null, 1, 1, 8, null) == -1
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.call("mr_occlusion_mask", null, null, null, null, 0, null, null, null, null, 1, 8, 8, 0.03, 0.99999, null)


def test_missing_library_fails_loudly(monkeypatch):
    from handobjectconsist_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "does_not_exist.so"))
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
        _lib.load()


def test_cpu_tensors_are_rejected_like_the_reference():
    import torch

    from handobjectconsist_amd.neurender import rasterize
    from handobjectconsist_amd.warping import imgflowarp

    with pytest.raises(TypeError):
        rasterize.rasterize_rgbad(torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 2, 2, 2, 3), 8, False)
    with pytest.raises(TypeError):
        rasterize.Rasterize(8, 0.1, 100, 1e-3, (0, 0, 0), True, True, True)(torch.zeros(1, 2, 3, 3),
                                                                            torch.zeros(1, 2, 2, 2, 2, 3))
    with pytest.raises(TypeError):
        imgflowarp.warp(torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "handobjectconsist_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f
                assert "liboracle" not in txt, f


def test_call_switches_to_the_device_of_its_stream(monkeypatch):
    """``_lib.call`` launches on the device its stream argument was taken from, not on whatever device
    happens to be current (tensors on cuda:1 while cuda:0 is current)."""
    import contextlib

    import torch

    from handobjectconsist_amd import _lib

    events = []

    class FakeLib:
        @staticmethod
        def mr_fake(*args):
            events.append(("launch", torch.cuda.current_device()))
            return 0

    state = {"current": 0}

    @contextlib.contextmanager
    def fake_device(idx):
        prev, state["current"] = state["current"], idx
        events.append(("enter", idx))
        try:
            yield
        finally:
            state["current"] = prev
            events.append(("exit", idx))

    monkeypatch.setattr(_lib, "load", lambda: FakeLib)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: state["current"])
    monkeypatch.setattr(torch.cuda, "device", fake_device)
    s1 = _lib._StreamArg(0)
    s1.device_index = 1
    _lib.call("mr_fake", None, 3, s1)
    assert events == [("enter", 1), ("launch", 1), ("exit", 1)]
    events.clear()
    s0 = _lib._StreamArg(0)
    s0.device_index = 0
    _lib.call("mr_fake", None, 3, s0)
    assert events == [("launch", 0)]


def _prototype(name):
    """[(kind, parameter name)] of a header prototype, kind in {"ptr", "stream", "int", "int64", "float"}"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"MR_API\s+(?:int64_t|int)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(","):
        words = decl.replace("*", " * ").split()
        kind = "stream" if "mr_stream_t" in words else "ptr" if "*" in words else \
            {"int": "int", "int64_t": "int64", "float": "float"}[[w for w in words[:-1] if w != "const"][0]]
        out.append((kind, words[-1]))
    return out


# An argument set every entry point below accepts: batch_size 2 at an 8 x 8 raster (one 32 x 8 tile per image), every
# pointer non-NULL (never dereferenced: each row of the table changes something that returns before the first HIP call).
_VALID = dict(batch_size=2, image_size=8, hit_image_size=8, height=8, width=8, jitter_channels=3, num_verts=4, num_faces=2,
              fill_back=1, split=1, flags=0, texel_layout=0, criterion=0, eps=1e-3, flow_bstride=128, workspace_bytes=1 << 30,
              list_capacity=4, tile_bound=-1)
_ZEROED = 4  # MR_FLAG_OUTPUT_ZEROED: no memset in front of the later checks
_SCATTER = ("mr_render_flow_backward", "mr_flow_pair_backward_tiles", "mr_flow_pair_backward_tiles_crit",
            "mr_flow_pair_backward_unit_tiles")
_PAIR_SCATTER = _SCATTER[1:]
_FLOW_FWD = ("mr_flow_pair_forward_tiles", "mr_flow_pair_forward_tiles_crit", "mr_flow_pair_forward_grad_tiles",
             "mr_flow_pair_forward_grad_tiles_crit")
_CONSIST = ("mr_pair_consist_forward", "mr_pair_consist_forward_crit", "mr_pair_consist_backward", "mr_pair_consist_backward_crit")
_CONSIST_TILES = ("mr_pair_consist_forward_tiles", "mr_pair_consist_forward_tiles_crit", "mr_pair_consist_backward_tiles",
                  "mr_pair_consist_backward_tiles_crit")
_CRIT = tuple(n for n in _SCATTER + _FLOW_FWD + _CONSIST + _CONSIST_TILES if n.endswith("_crit"))
_WITH_WORKSPACE = _FLOW_FWD + _CONSIST[:2] + _CONSIST_TILES[:2]

# (entry points, overrides of _VALID -- None = NULL --, expected return)
_VALIDATION_TABLE = [
    # ---- tile scatter backward (raster_bwd_vc.hip) ----
    (_SCATTER, dict(batch_size=-1), -1),
    (_SCATTER, dict(num_verts=-1), -1),
    (_SCATTER, dict(num_faces=-1), -1),
    (_SCATTER, dict(image_size=0), -1),
    (_SCATTER, dict(texel_layout=63), -1),
    (_SCATTER, dict(texel_layout=0b000101), -1),
    (_SCATTER, dict(grad_vcolors=None), -1),
    (_SCATTER, dict(batch_size=0), 0),
    (_SCATTER, dict(batch_size=0, grad_vcolors=None), 0),
    (_SCATTER, dict(num_verts=0), 0),
    (_SCATTER, dict(num_verts=0, grad_vcolors=None, face_index_map=None), 0),
    (_PAIR_SCATTER, dict(batch_size=3), -1),
    (_PAIR_SCATTER, dict(batch_size=3, num_verts=0), -1),
    (_PAIR_SCATTER, dict(tile_hit=None), -1),
    (_PAIR_SCATTER, dict(sums=None), -1),
    (_PAIR_SCATTER, dict(grad_loss_fwd=None), -1),
    (_PAIR_SCATTER, dict(grad_loss_fwd=None, batch_size=0), 0),
    (_PAIR_SCATTER, dict(width=1), -1),
    (_PAIR_SCATTER, dict(height=0), -1),
    (_PAIR_SCATTER, dict(height=9), -1),
    (_PAIR_SCATTER, dict(width=9), -1),
    (_PAIR_SCATTER, dict(width=1, flags=_ZEROED, image_size=10), -1),
    (_PAIR_SCATTER, dict(flags=_ZEROED, num_faces=0), 0),
    (_PAIR_SCATTER, dict(flags=_ZEROED, num_faces=0, vertex_id_map=None, eps=0.0, image_size=10), 0),
    (_PAIR_SCATTER, dict(flags=_ZEROED, vertex_id_map=None), -1),
    (_PAIR_SCATTER, dict(flags=_ZEROED, vertex_id_map=None, image_size=10), -1),
    (_SCATTER, dict(flags=_ZEROED, face_index_map=None), -1),
    (_SCATTER, dict(flags=_ZEROED, weight_map=None), -1),
    (_SCATTER, dict(flags=_ZEROED, eps=0.0), -1),
    (_SCATTER, dict(flags=_ZEROED, eps=0.0, image_size=10), -1),
    (_SCATTER, dict(flags=_ZEROED, image_size=10), -2),
    (_SCATTER, dict(flags=_ZEROED, image_size=10, grad_loss_bwd=None, grad_bound=None, scatter_work=None), -2),
    (_SCATTER, dict(flags=_ZEROED, num_verts=100000), -2),
    (_SCATTER, dict(flags=_ZEROED, image_size=4100, height=4100, width=4100), -2),  # more than 4096 tiles per image
    (("mr_render_flow_backward",), dict(flags=_ZEROED, batch_size=3, image_size=10), -2),  # (no pairs: odd batches pass)
    (("mr_render_flow_backward",), dict(flags=_ZEROED, num_faces=0, face_index_map=None), 0),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, grad_rgb_img=None), -2),  # the flow-gradient form
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, grad_flow=None), -2),  # (colour form: not looked at)
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, grad_flow=None), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, mask_pre=None), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, mask_x_lo=None), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, occl=None), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, height=9), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, width=0), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, split=3), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, split=-1), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, mask_x_hi=None), -1),
    (("mr_render_flow_backward",), dict(grad_rgb_img=None, mask_x_hi=None, split=2, flags=_ZEROED, image_size=10), -2),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, height=99, width=0, split=7), -2),  # (colour form)
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, vertex_id_map=None), -2),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, vertex_id_map=None, verts=None), -1),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, vertex_id_map=None, faces_idx=None), -1),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, vertex_id_map=None, depth_img=None), -1),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, image_size=10, verts=None, faces_idx=None, depth_img=None), -2),
    # (three table entries per vertex in the colour form, two in the flow-gradient form: 60 KB of 16-byte entry pairs)
    (("mr_render_flow_backward",), dict(flags=_ZEROED, num_verts=2561), -2),
    (("mr_render_flow_backward",), dict(flags=_ZEROED, num_verts=3841, grad_rgb_img=None), -2),
    (_PAIR_SCATTER, dict(flags=_ZEROED, num_verts=3841), -2),
    (_PAIR_SCATTER[:2], dict(jitter_channels=2), -1),
    (_PAIR_SCATTER[:2], dict(jitter_channels=2, batch_size=0), 0),
    (_PAIR_SCATTER[:2], dict(flows=None), -1),
    (_PAIR_SCATTER[:2], dict(image_ref=None), -1),
    (_PAIR_SCATTER[:2], dict(jitter=None), -1),
    (_PAIR_SCATTER[:2], dict(mask_x_hi=None), -1),
    (_PAIR_SCATTER[:2], dict(occl=None), -1),
    (_PAIR_SCATTER[:2], dict(grad_flow_scratch=None), -1),
    (("mr_flow_pair_backward_unit_tiles",), dict(unit_grad=None), -1),
    (("mr_flow_pair_backward_unit_tiles",), dict(unit_grad_max=None), -1),
    (("mr_flow_pair_backward_unit_tiles",), dict(grad_loss_fwd=None, num_verts=0), 0),
    (("mr_flow_pair_backward_unit_tiles",), dict(grad_loss_fwd=None, batch_size=-2), -1),
    # ---- the criterion comes first wherever there is one ----
    (_CRIT, dict(criterion=2), -1),
    (_CRIT, dict(criterion=-1), -1),
    (_CRIT, dict(criterion=2, batch_size=0, list_capacity=0), -1),
    (_CRIT, dict(criterion=1, batch_size=0, list_capacity=0), 0),
    # ---- flow-pair forward over the tile list (warp_tiles.hip) ----
    (_FLOW_FWD, dict(mask_flow1=None), -1),
    (_FLOW_FWD, dict(mask_flow2=None), -1),
    (_FLOW_FWD, dict(flow12=None), -1),
    (_FLOW_FWD, dict(flow21=None), -1),
    (_FLOW_FWD, dict(occl1=None), -1),
    (_FLOW_FWD, dict(occl2=None), -1),
    (_FLOW_FWD, dict(flow_out12=None), -1),
    (_FLOW_FWD, dict(flow_out21=None), -1),
    (_FLOW_FWD, dict(batch_size=-1), -1),
    (_FLOW_FWD, dict(image_size=0), -1),
    (_FLOW_FWD, dict(flow_bstride=127), -1),
    (_FLOW_FWD, dict(tile_hit1=None), -1),
    (_FLOW_FWD, dict(tile_hit2=None), -1),
    (_FLOW_FWD, dict(height=9), -1),
    (_FLOW_FWD, dict(width=9), -1),
    (_FLOW_FWD, dict(batch_size=0, list_capacity=0), 0),
    (_FLOW_FWD, dict(batch_size=0, list_capacity=0, workspace_bytes=0, flow12_scale=None, flow21_scale=None, loss_fwd=None,
                     loss_bwd=None, loss_sum=None, scatter_work=None), 0),
    (_FLOW_FWD, dict(batch_size=0, list_capacity=0, occl1=None), -1),
    (_FLOW_FWD[2:], dict(unit_grad=None), -1),
    (_FLOW_FWD[2:], dict(unit_grad_max=None), -1),
    (_FLOW_FWD[2:], dict(unit_grad=None, batch_size=0, list_capacity=0), -1),
    # ---- what the pair-loss launchers share (warp.hip, warp_tiles.hip) ----
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(image_ref=None), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(image=None), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(jitter_ref=None), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(jitter=None), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(jitter_channels=2), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(jitter_channels=0), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(jitter_channels=2, batch_size=0, list_capacity=0), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(width=1), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(width=1, batch_size=0, list_capacity=0), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(height=0), -1),
    (_FLOW_FWD + _CONSIST + _CONSIST_TILES, dict(sums=None), -1),
    (_CONSIST + _CONSIST_TILES, dict(flow12=None), -1),
    (_CONSIST + _CONSIST_TILES, dict(flow21=None), -1),
    (_CONSIST + _CONSIST_TILES, dict(batch_size=-1), -1),
    (_CONSIST + _CONSIST_TILES, dict(hit_image_size=7), -1),
    (_CONSIST + _CONSIST_TILES, dict(batch_size=0, list_capacity=0), 0),
    (_CONSIST + _CONSIST_TILES, dict(height=32768, width=32768, hit_image_size=32768, batch_size=0, list_capacity=0), -1),
    (_WITH_WORKSPACE, dict(workspace=None), -1),
    (_WITH_WORKSPACE, dict(workspace_bytes=0), -1),
    (_WITH_WORKSPACE, dict(workspace_bytes=0, batch_size=0, list_capacity=0), 0),
    (_CONSIST[2:] + _CONSIST_TILES[2:], dict(grad_loss_fwd=None), -1),
    (_CONSIST[2:] + _CONSIST_TILES[2:], dict(grad_flow12=None), -1),
    (_CONSIST[2:] + _CONSIST_TILES[2:], dict(grad_flow21=None), -1),
    (_CONSIST[2:] + _CONSIST_TILES[2:], dict(grad_loss_bwd=None, grad_max=None, batch_size=0, list_capacity=0), 0),
    (_CONSIST, dict(tile_hit12=None, tile_hit21=None, hit_image_size=0, batch_size=0), 0),  # (coverage bytes are optional)
    (_CONSIST, dict(tile_hit21=None, hit_image_size=7), -1),
    (_CONSIST, dict(height=32768, width=32768, hit_image_size=32768, batch_size=-1), -1),
    (_CONSIST[:2], dict(full_mask1=None, full_mask2=None, warp_mask1=None, warp_mask2=None, warp1=None, warp2=None, diff1=None,
                        diff2=None, loss_fwd=None, loss_bwd=None, batch_size=0), 0),
    (_FLOW_FWD + _CONSIST_TILES, dict(list_header=None), -1),
    (_FLOW_FWD + _CONSIST_TILES, dict(list_entries=None), -1),
    (_FLOW_FWD + _CONSIST_TILES, dict(list_capacity=3), -1),
    (_FLOW_FWD + _CONSIST_TILES, dict(list_capacity=8), -1),
    (_FLOW_FWD + _CONSIST_TILES, dict(batch_size=0), -1),  # (the capacity is checked before the empty batch returns)
    (_CONSIST_TILES, dict(tile_hit12=None), -1),
    (_CONSIST_TILES, dict(tile_hit21=None), -1),
    # (2 B tiles_x tiles_y beyond 31 bits)
    (_FLOW_FWD + _CONSIST_TILES, dict(batch_size=1 << 20, image_size=4096, hit_image_size=4096, flow_bstride=1 << 26,
                                      list_capacity=(2 << 20) * 128 * 512), -1),
]


def test_validation_returns_of_the_pair_launchers():
    """What the frame-pair path's entry points answer to arguments they refuse -- or accept without work -- before any HIP
    call: MR_ERR_BADARG (-1), MR_ERR_NOTIMPL (-2) or MR_OK (0), entry point by entry point and in each one's own order of
    checks (rows with two faults pin which one is seen first).  Needs no device."""
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    protos = {name: _prototype(name) for names, _, _ in _VALIDATION_TABLE for name in names}
    ran = 0
    for names, over, want in _VALIDATION_TABLE:
        assert set(over) <= {p for name in names for _, p in protos[name]}, over  # (a misspelt parameter)
        for name in names:
            proto = protos[name]
            pnames = {p for _, p in proto}
            # (a row shared by several entry points may name parameters only some of them have; each has at least one)
            mine = {k: v for k, v in over.items() if k in pnames}
            assert mine, (name, over)
            args = []
            for kind, p in proto:
                if kind == "stream":
                    args.append(None)
                elif kind == "ptr":
                    args.append(mine.get(p, 0x1000))
                elif kind == "float":
                    args.append(float(mine.get(p, _VALID.get(p, 0.5))))
                else:
                    assert p in mine or p in _VALID, (name, p)
                    args.append(int(mine.get(p, _VALID.get(p))))
            got = getattr(lib, name)(*args)
            assert got == want, f"{name}({over}) returned {got}, expected {want}"
            ran += 1
    assert ran > 500
