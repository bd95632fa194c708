"""``ResNet18Features`` with the stem's convolution inside the stem node (``synthnet.USE_STEM_WRW``) against the composed
path, from equal weights on a [4, 3, 64, 64] batch: features and every parameter gradient except ``conv1.weight.grad``
bit for bit; ``conv1.weight.grad`` -- an fp32 sum of the same terms in another order -- within twice the composed path's
own error against an fp64 CPU ``conv2d_weight`` over the same gradient map (the bound of tests/test_gpu_stem_wrw.py).  An
image that requires a gradient takes the composed path, and its gradient is what it was.

MIOpen's default solvers add with float atomics and give the composed path other bits from run to run, so both tests hold
it to its deterministic solvers (``torch.backends.cudnn.deterministic``), as ``bench.py --dump-outputs`` does."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def deterministic_convolutions():
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def _net(cuda):
    from handobjectconsist_amd.models import synthnet

    torch.manual_seed(11)
    net = synthnet.ResNet18Features()
    g = torch.Generator().manual_seed(12)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=g)
            m.bias.data = 0.2 * torch.randn(m.bias.shape, generator=g)
            m.running_mean = 0.2 * torch.randn(m.bias.shape, generator=g)
            m.running_var = 0.5 + torch.rand(m.bias.shape, generator=g)
    return net.to(cuda).eval()


def _step(net, image, switch, monkeypatch):
    from handobjectconsist_amd.models import synthnet

    monkeypatch.setattr(synthnet, "USE_STEM_WRW", switch)
    net = copy.deepcopy(net)
    out = net(image)
    out.square().sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {n: p.grad for n, p in net.named_parameters()}


def test_trunk_with_and_without_the_switch(cuda, monkeypatch):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.models import synthnet
    from handobjectconsist_amd.nn import frozen_bn

    assert synthnet.USE_STEM_WRW is True and synthnet.USE_HIP_BN and synthnet.USE_CHANNELS_LAST
    net = _net(cuda)
    image = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(13)).to(cuda)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, *a: (calls.append(n), real(n, *a))[1])
    out_on, g_on = _step(net, image, True, monkeypatch)
    assert "mr_stem_conv_wrw" in calls and "mr_stem_pool_param_grads" in calls and "mr_stem_pool_backward" not in calls
    calls.clear()
    out_off, g_off = _step(net, image, False, monkeypatch)
    assert "mr_stem_conv_wrw" not in calls and "mr_stem_pool_backward" in calls
    assert torch.equal(out_on, out_off)
    assert set(g_on) == set(g_off)
    for n in g_off:
        assert g_on[n] is not None and g_on[n].shape == g_off[n].shape and g_on[n].stride() == g_off[n].stride(), n
        if n != "conv1.weight":
            assert torch.equal(g_on[n], g_off[n]), n
    # conv1.weight.grad against fp64 over the gradient map of the composed path (taken where conv1's output enters the
    # stem node; with deterministic solvers it is the map the new path's kernel forms in LDS, every later gradient being
    # bit-equal).  The yardstick is the composed path as the trunk runs it, MIOpen's default solver choice, measured against
    # the map of its own run; the figure with the deterministic solver is printed next to it.
    def composed(deterministic):
        maps = []

        def keep_gradient(module, inputs, output):
            output.register_hook(lambda g: maps.append(g.detach()))

        torch.backends.cudnn.deterministic = deterministic
        monkeypatch.setattr(synthnet, "USE_STEM_WRW", False)
        ref_net = copy.deepcopy(net)
        h = ref_net.conv1.register_forward_hook(keep_gradient)
        ref_net(image).square().sum().backward()
        h.remove()
        torch.cuda.synchronize()
        torch.backends.cudnn.deterministic = True
        ref = torch.nn.grad.conv2d_weight(image.cpu().double(), (64, 3, 7, 7), maps[0].cpu().double().contiguous(), stride=2, padding=3)
        return ref, ref_net.conv1.weight.grad.cpu().double()

    rel = lambda got, ref: float((got - ref).abs().max()) / float(ref.abs().max())
    ref, got_det = composed(True)
    assert torch.equal(got_det.float(), g_off["conv1.weight"].cpu())
    err_on, err_det = rel(g_on["conv1.weight"].cpu().double(), ref), rel(got_det, ref)
    err_off = rel(*composed(False)[::-1])
    print(f"STEM-WRW trunk [4,3,64,64]: max|gW| {float(ref.abs().max()):.4g}  new kernel {err_on:.3e}  composed path {err_off:.3e}"
          f"  (composed path, deterministic solver {err_det:.3e})")
    assert err_on <= 2 * err_off


def test_an_image_that_requires_a_gradient_takes_the_composed_path(cuda, monkeypatch):
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.models import synthnet

    net = _net(cuda)
    base = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(14)).to(cuda)
    grads = {}
    for switch in (True, False):
        monkeypatch.setattr(synthnet, "USE_STEM_WRW", switch)
        calls = []
        real = _lib.call
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "call", lambda n, *a: (calls.append(n), real(n, *a))[1])
            image = base.clone().requires_grad_(True)
            n2 = copy.deepcopy(net)
            n2(image).square().sum().backward()
            torch.cuda.synchronize()
        assert "mr_stem_conv_wrw" not in calls and "mr_stem_pool_backward" in calls
        grads[switch] = (image.grad, n2.conv1.weight.grad)
    assert grads[True][0] is not None and torch.equal(grads[True][0], grads[False][0])
    assert torch.equal(grads[True][1], grads[False][1])
