"""Generate tests/golden/trunk_glue_bits.json: SHA-256 digests of what the trunk's glue kernels (csrc/frozen_bn.hip,
csrc/stem_pool.hip) compute on random normal data, taken through the raw entry points on an MI355X.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trunk_glue.py [output path]

The exact tests (tests/test_gpu_trunk_exact.py, test_gpu_block_tail.py, test_gpu_stem_records.py) use operands whose sums
are exact in fp32 and so cannot see a changed summation order or expression shape.  Here the data are drawn as
``_randn_case`` of tests/test_gpu_stem_records.py draws them -- CPU generator, normal values rounded to bf16, var in
[0.05, 2.05], eps = 1e-5 -- so products and sums round and every order shows in the bits of grad_weight / grad_bias.

The file is a record of the kernels as they were BEFORE their mechanisms moved into csrc/bn_device.hpp (the library's
``build.source_hash()`` at that commit is stored with it).  It is not regenerated from later code: a digest that
differs is a changed result.  tests/test_gpu_trunk_glue_bits.py imports the cases and the runner from this file.

Cases (each in fp32 and bf16): the smallest shapes that reach every kernel instantiation and every reduction stage.
bn_act NCHW scalar path (HW % 4 != 0) with ReLU + residual and without either; NCHW vector path with bn_split = 6 slots
per channel; bn_act and bn_add_bn_act channels-last with 16 rows per workgroup in one trip and with one row per workgroup
in more than 2048 workgroups (second grid-stride trip), bn_add_bn_act also with only grad_weight_d requested; the stem
in layout 0 with W % 4 != 0 and with several tiles per plane, in layouts 1 and 2 on two small shapes and on one whose
4225 pooled pixels / quads exceed 4096 workgroups of one row; one single-gradient arrival per family.
"""
import collections
import functools
import hashlib
import json
import os
import sys

import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "trunk_glue_bits.json")
EPS = 1e-5
FP32, BF16 = torch.float32, torch.bfloat16
DTYPES = {"fp32": FP32, "bf16": BF16}

Case = collections.namedtuple("Case", "name family shape opts")

SMALL, WIDE, ODD = (6, 64, 32, 32), (3, 1024, 27, 27), (5, 16, 17, 30)
CASES = [
    Case("bn_act_nchw_scalar_relu_residual", "bn_act", ODD, dict(cl=0, relu=1, residual=True)),
    Case("bn_act_nchw_scalar_plain", "bn_act", ODD, dict(cl=0, relu=0, residual=False)),
    Case("bn_act_nchw_vector_split6", "bn_act", SMALL, dict(cl=0, relu=1, residual=True)),
    Case("bn_act_nhwc_one_trip", "bn_act", SMALL, dict(cl=1, relu=1, residual=True)),
    Case("bn_act_nhwc_two_trips", "bn_act", WIDE, dict(cl=1, relu=1, residual=True)),
    Case("bn_act_nhwc_single_gradient", "bn_act", SMALL, dict(cl=1, relu=1, residual=True, single=True)),
    Case("bn_add_one_trip", "bn_add", SMALL, dict()),
    Case("bn_add_two_trips", "bn_add", WIDE, dict()),
    Case("bn_add_one_trip_only_grad_weight_d", "bn_add", SMALL, dict(only_wd=True)),
    Case("bn_add_two_trips_only_grad_weight_d", "bn_add", WIDE, dict(only_wd=True)),
    Case("bn_add_single_gradient", "bn_add", SMALL, dict(single=True)),
    Case("stem_layout0_odd_width", "stem", ODD, dict(layout=0)),
    Case("stem_layout0_tile_seams", "stem", (2, 8, 70, 140), dict(layout=0)),
    Case("stem_layout0_single_gradient", "stem", ODD, dict(layout=0, single=True)),
]
for _layout in (1, 2):
    CASES += [Case(f"stem_layout{_layout}_{'x'.join(map(str, s))}", "stem", s, dict(layout=_layout))
              for s in (ODD, SMALL, (1, 1024, 129, 129))]
CASES.append(Case("stem_layout2_single_gradient", "stem", ODD, dict(layout=2, single=True)))


def _pooled(shape):
    N, C, H, W = shape
    return (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


@functools.lru_cache(maxsize=4)
def draw(family, shape):
    """CPU tensors of a family's case, NCHW, fp32 holding bf16 values (the same data for both activation types)"""
    g = torch.Generator().manual_seed(sum(shape) + {"bn_act": 101, "bn_add": 202, "stem": 1}[family])
    C = shape[1]
    rn = lambda s: torch.randn(s, generator=g)
    bf = lambda t: t.bfloat16().float()
    params = lambda: dict(weight=rn(C) * 0.5 + 1.0, bias=rn(C) * 0.3, mean=rn(C) * 0.4, var=torch.rand(C, generator=g) * 2 + 0.05)
    gshape = _pooled(shape) if family == "stem" else shape
    d = dict(x=bf(rn(shape)), gy=bf(rn(gshape)), gy2=bf(rn(gshape)), **params())
    if family == "bn_act":
        d["residual"] = bf(rn(shape))
    if family == "bn_add":
        d["xd"] = bf(rn(shape))
        d.update({k + "_d": v for k, v in params().items()})
    return d


def digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == BF16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def run_case(case, dtype, dev):
    """One forward + backward through the C entry points.  Returns (inputs, outputs): dicts name -> device tensor as the
    kernels saw / left it.  Output buffers start as zeros so that bytes no kernel writes (record padding) are defined."""
    from handobjectconsist_amd import _lib

    P, st, lib = _lib.ptr, _lib.stream_ptr(dev), _lib.load()
    d, o = draw(case.family, case.shape), case.opts
    N, C, H, W = case.shape
    code = 0 if dtype == FP32 else 1
    cl = o.get("cl", 1) if case.family != "stem" else int(o["layout"] != 0)
    act = lambda t: (t.permute(0, 2, 3, 1) if cl else t).contiguous().to(dev, dtype)   # memory order the kernels read
    vec = lambda k: d[k].to(dev).float().contiguous()
    zeros = lambda like: torch.zeros_like(like)
    ins = {k: act(d[k]) for k in ("x", "gy", "gy2", "residual", "xd") if k in d}
    ins.update({k: vec(k) for k in d if d[k].dim() == 1})
    if o.get("single"):
        del ins["gy2"]
    if case.family == "bn_act" and not o["residual"]:
        del ins["residual"]
    x, gy, gy2 = ins["x"], ins["gy"], ins.get("gy2")
    chan = [ins[k] for k in ("weight", "bias", "mean", "var")]
    out = {}
    if case.family == "bn_act":
        r = ins.get("residual")
        out["y"], out["grad_x"] = zeros(x), zeros(x)
        if r is not None:
            out["grad_residual"] = zeros(x)
        out["grad_weight"], out["grad_bias"] = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        _lib.call("mr_bn_act_forward", P(x), P(r), *map(P, chan), EPS, o["relu"], code, cl, P(out["y"]), N, C, H * W, st)
        wbytes = int(lib.mr_bn_act_backward_workspace_bytes(N, C))
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        _lib.call("mr_bn_act_backward", P(gy), P(gy2), P(x), P(r), *map(P, chan), EPS, o["relu"], code, cl, P(out["grad_x"]),
                  P(out.get("grad_residual")), P(out["grad_weight"]), P(out["grad_bias"]), P(work), wbytes, N, C, H * W, st)
    elif case.family == "bn_add":
        xd = ins["xd"]
        chan_d = [ins[k + "_d"] for k in ("weight", "bias", "mean", "var")]
        out["y"], out["grad_x"], out["grad_xd"] = zeros(x), zeros(x), zeros(x)
        for k in (("grad_weight_d",) if o.get("only_wd") else ("grad_weight", "grad_bias", "grad_weight_d", "grad_bias_d")):
            out[k] = torch.zeros(C, device=dev)
        _lib.call("mr_bn_add_bn_act_forward", P(x), P(xd), *map(P, chan), EPS, *map(P, chan_d), EPS, code, P(out["y"]),
                  N, C, H * W, st)
        wbytes = int(lib.mr_bn_add_bn_act_backward_workspace_bytes(N, C))
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        _lib.call("mr_bn_add_bn_act_backward", P(gy), P(gy2), P(x), P(xd), *map(P, chan), EPS, *map(P, chan_d), EPS, code,
                  P(out["grad_x"]), P(out["grad_xd"]), P(out.get("grad_weight")), P(out.get("grad_bias")),
                  P(out.get("grad_weight_d")), P(out.get("grad_bias_d")), P(work), wbytes, N, C, H * W, st)
    else:
        layout = o["layout"]
        out["y"], out["grad_x"] = zeros(gy), zeros(x)
        out["grad_weight"], out["grad_bias"] = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        rec = None
        if layout:   # layout 1: the arg-max codes; layout 2: the records (x - mean, then the codes)
            rbytes = int(lib.mr_stem_pool_records_bytes(N, C, H, W)) if layout == 2 else gy.numel()
            rec = out["records"] = torch.zeros(rbytes, dtype=torch.uint8, device=dev)
        _lib.call("mr_stem_pool_forward", P(x), *map(P, chan), EPS, code, layout, P(out["y"]), P(rec), N, C, H, W, st)
        wbytes = int(lib.mr_stem_pool_backward_workspace_bytes(N, C, H, W))
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        _lib.call("mr_stem_pool_backward", P(gy), P(gy2), P(None if layout == 2 else x), P(rec), *map(P, chan), EPS, code,
                  layout, P(out["grad_x"]), P(out["grad_weight"]), P(out["grad_bias"]), P(work), wbytes, N, C, H, W, st)
    torch.cuda.synchronize(dev)
    return ins, out


def digests(case, dtype, dev):
    ins, out = run_case(case, dtype, dev)
    return {k: digest(v) for k, v in ins.items()}, {k: digest(v) for k, v in out.items()}


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    from handobjectconsist_amd import build

    dev = torch.device("cuda:0")
    res = {"source_hash": build.source_hash(), "device": torch.cuda.get_device_name(dev), "cases": {}}
    for case in CASES:
        for tag, dtype in DTYPES.items():
            i, o = digests(case, dtype, dev)
            res["cases"][f"{case.name}-{tag}"] = {"inputs": i, "outputs": o}
            print(case.name, tag, " ".join(f"{k}={v[:8]}" for k, v in o.items()))
    out_path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{out_path}: {len(res['cases'])} cases, library source hash {res['source_hash'][:12]}")


if __name__ == "__main__":
    main()
