"""Forward + backward of the FPHAB adaptor stage at the trainer's size (B = 192 hands of one step, V = 778, J = 21, centre 9):
    (a) the HIP stage: mr_mano_adapt_forward / _backward through models/manoadapt.adapt_hip
    (b) the reference's formulation in stock PyTorch ops: transpose, Linear, index, two subtractions, and their autograd
    python scripts/mano_adapt_timing.py [--batch 192] [--iters 200] [--windows 5] [--weight-grad]
The weight is frozen, as in the network, unless --weight-grad.  Needs a GPU.  Both variants get the same seeded inputs and
incoming gradients; their results are compared first (max |a - b| is printed).  Figures, per forward + backward:
    graph_us   device events around ``--iters`` replays of a hipGraph that holds one forward + backward (device time: the
               kernels and the gaps the device itself leaves between them), median and best of ``--windows`` windows, the two
               variants alternating
    eager_us   the same events around ``--iters`` eager calls: what a training step sees, launch costs of the host included
    kernels    device kernels per forward + backward, counted by torch.profiler in a pass of its own (None where the profiler
               gives no device events)
Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--weight-grad", action="store_true")
    a = ap.parse_args()
    import torch

    from handobjectconsist_amd.models import manoadapt, synthnet

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    B, center = a.batch, 9
    g = torch.Generator().manual_seed(0)
    layer = synthnet.SynthManoLayer().to(dev)
    with torch.no_grad():
        verts = layer(0.4 * torch.randn(B, 18, generator=g).to(dev), torch.randn(B, 10, generator=g).to(dev))[0].contiguous()
    adaptor = manoadapt.ManoAdaptor(layer).to(dev)
    weight = adaptor.adaptor.weight.detach().clone().requires_grad_(a.weight_grad)
    gv, gj = torch.randn(B, 778, 3, generator=g).to(dev), torch.randn(B, 21, 3, generator=g).to(dev)
    leaves = lambda v: [v, weight] if a.weight_grad else [v]

    def hip():
        v = verts.detach().requires_grad_(True)
        vo, jo = manoadapt.adapt_hip(v, weight, center)
        return [vo, jo] + list(torch.autograd.grad([vo, jo], leaves(v), [gv, gj]))

    def stock():
        v = verts.detach().requires_grad_(True)
        j = torch.nn.functional.linear(v.transpose(2, 1), weight).transpose(1, 2)
        c = j[:, center].unsqueeze(1)
        jo, vo = j - c, v - c
        return [vo, jo] + list(torch.autograd.grad([vo, jo], leaves(v), [gv, gj]))

    variants = {"hip": hip, "stock": stock}
    first = {name: [t.detach().clone() for t in fn()] for name, fn in variants.items()}
    torch.cuda.synchronize()
    diff = [float((x - y).abs().max()) for x, y in zip(first["hip"], first["stock"])]

    def window(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters

    graphs = {}
    for name, fn in variants.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=side):
            keep = fn()  # noqa: F841  (the graph's pool holds the results)
    times = {f"{name}_{kind}": [] for name in variants for kind in ("graph", "eager")}
    for w in range(a.windows + 1):  # (the first window of each is a warm-up)
        for name, fn in variants.items():
            for kind, run in (("graph", graphs[name].replay), ("eager", fn)):
                t = window(run)
                if w:
                    times[f"{name}_{kind}"].append(t)
    kernels = {}
    for name, fn in variants.items():
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
            kernels[name] = round(n / 10, 1) if n else None
        except Exception as exc:  # noqa: BLE001  (a count is not worth a failed measurement)
            kernels[name] = None
            print(f"profiler pass failed for {name}: {exc}", file=sys.stderr)
    out = {"batch": B, "iters": a.iters, "windows": a.windows, "weight_grad": a.weight_grad, "max_abs_diff_hip_vs_stock": diff, "kernels": kernels}
    for key, vals in times.items():
        out[key + "_us_median"] = round(float(np.median(vals)), 2)
        out[key + "_us_min"] = round(float(np.min(vals)), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
