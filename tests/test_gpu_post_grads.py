"""mr_meshreg_post_forward / _backward (csrc/meshreg_post.hip) called directly on random vertices and joints, every buffer
from tests/guarded_alloc.py: all five outputs and all four gradients, element by element and normalised per sample, against
``oracle/geom_grad_ref.post_forward`` in float64 with autograd -- a restatement of recover_3d_proj (focal = K[0,0] alone),
manopth's quaternion Rodrigues and (K p)[:2] / (K p)[2] that calls nothing of the product.  test_gpu_warp.py's
``test_meshreg_post_hip_matches_torch_ops`` compares with the fp32 PyTorch path on the same GPU, at fx == fy, zero skew and a
third row (0, 0, 1); here K has fx != fy, a skew, an off-centre principal point and, in each case's last sample, a third
row (0.02, -0.03, 1).

Shapes (tests/geom_grad_cases.POST_SHAPES): one object vertex; the trainer's; hand and object points both ending on the
256-point block boundary; one object vertex in a second block; joints straddling the boundary; no object; no hand.  Object
rotations per sample: zero, (1e-6, 0, 0), 3.1 rad, 6.4 rad, two random.  Gradient subsets: all five, each alone, both
projections, none.

Tolerance: four times the error of ``post_forward`` on float32 tensors on the CPU in the same case and tensor;
tests/test_geom_grad_ref_host.py holds that yardstick to 2.5e-6 (gradients) / 1e-6 (values).  Every case prints
``tensor yardstick/kernel`` on one line (profiles/geometry_grads.txt).

Measured on an MI355X (host: EPYC 9575F), largest kernel / yardstick ratio per tensor: the five outputs 1.00 .. 1.56
(objverts2d), grad verts_mm 1.00, grad joints_mm 1.14, grad scaletrans 1.52, grad st_obj 1.91; the per-sample sums over
Vo >= 256 dense weights stay below 2 x, so the rule's 16 x for many-term sums is not used.

These tests found the centre adjoint of ``post_backward_finish_kernel`` a rounding step less accurate than need be ((1, 778,
21, 1) with joints3d alone in the loss, grad scaletrans: yardstick 1.62e-8, kernel 7.39e-8 = 4.56 x); computed in double, once
per sample, it reads 1.62e-8 / 1.62e-8."""
import pytest
import torch

from tests import geom_grad_cases as C
from tests import guarded_alloc as G

pytestmark = pytest.mark.gpu

MR_OK, MR_ERR_BADARG = 0, -1
OUT_SHAPES = lambda B, Vh, J, Vo: [(B, Vh, 3), (B, J, 3), (B, J, 2), (B, Vo, 3), (B, Vo, 2)]


def _ptr(t):
    """a part with no elements is passed as a null pointer"""
    from handobjectconsist_amd import _lib

    return _lib.ptr(t) if t is not None and t.numel() else None


def _consts():
    tf, sf, off_z, (rw, rh) = C.POST_CONSTS
    return tf, sf, off_z, rw, rh


def run_post(cuda, shape, subset):
    """forward + backward through the C-ABI on guarded buffers -> (five outputs, four gradients) as tensors.  Outputs and
    gradients start as NaN (the allocator's fill), so an element no thread writes fails the comparison."""
    from handobjectconsist_amd import _lib

    alloc = G.GuardedAllocator(cuda)
    with alloc:
        ins = [alloc.guard(torch.from_numpy(a)) for a in C.post_inputs(shape)]
        outs = [torch.empty(s, dtype=torch.float32, device=cuda) for s in OUT_SHAPES(*shape)]
        _lib.call("mr_meshreg_post_forward", *[_ptr(x) for x in ins], *_consts(), *[_ptr(o) for o in outs], *shape,
                  _lib.stream_ptr(cuda))
        weights = C.post_weights(shape)
        gin = [alloc.guard(torch.from_numpy(weights[k])) if k in subset else None for k in range(5)]
        work = torch.empty((shape[0] * 15,), dtype=torch.float32, device=cuda)
        grads = [torch.empty_like(x) for x in ins[:4]]
        _lib.call("mr_meshreg_post_backward", *[_ptr(x) for x in ins], *_consts(), *[_ptr(g) for g in gin], _ptr(work),
                  *[_ptr(g) for g in grads], *shape, _lib.stream_ptr(cuda))
    damage = alloc.check()
    assert not damage, damage
    return outs, grads


CASES = [(s, sub) for s in C.POST_SHAPES for sub in C.POST_SUBSETS]


@pytest.mark.parametrize("shape,subset", CASES, ids=[f"{'x'.join(map(str, s))}-grads{''.join(map(str, sub)) or 'none'}" for s, sub in CASES])
def test_every_output_and_gradient_element_matches_float64(cuda, shape, subset):
    outs, grads = run_post(cuda, shape, subset)
    (outs64, grads64), (outs32, grads32) = C.post_reference(shape, subset), C.post_reference(shape, subset, torch.float32)
    report = C.Report(f"post {shape} grads of {subset}")
    for name, got, yard, ref in zip(C.POST_OUTPUTS, outs, outs32, outs64):
        assert tuple(got.shape) == ref.shape
        report.add(name, got.cpu().numpy(), yard, ref, C.MAX_EY_VALUE)
    for name, got, yard, ref in zip(C.POST_GRADS, grads, grads32, grads64):
        report.add("grad " + name, got.cpu().numpy(), yard, ref, C.MAX_EY_GRAD)
    report.finish()
    B, Vh, J, Vo = shape
    if Vo == 0 or not set(subset) & {3, 4}:
        assert not bool((grads[3] != 0).any()), "grad st_obj with nothing of the object in the loss"
    if Vh + J == 0 or not set(subset) & {0, 1, 2}:
        assert not bool((grads[2] != 0).any()), "grad scaletrans with nothing of the hand in the loss"
    if not subset:
        assert all(not bool((g != 0).any()) for g in grads)


@pytest.mark.parametrize("shape", [s for s in C.POST_SHAPES if s[3] <= 256 and s[1] + s[2] <= 256], ids=str)
def test_one_block_per_sample_gives_the_same_bits_twice(cuda, shape):
    """a sample whose points fit one block adds ONE float atomic per sum to a zeroed workspace: nothing to reorder"""
    first, second = run_post(cuda, shape, (0, 1, 2, 3, 4)), run_post(cuda, shape, (0, 1, 2, 3, 4))
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert torch.equal(a, b)


def test_refusals_launch_nothing(cuda):
    """each refusal returns MR_ERR_BADARG with every output still holding its fill; B = 0 is MR_OK and writes nothing either"""
    from handobjectconsist_amd import _lib

    lib, shape = _lib.load(), (2, 5, 3, 4)
    B, Vh, J, Vo = shape
    ins = [torch.from_numpy(a).to(cuda) for a in C.post_inputs(shape)]
    outs = [torch.full(s, 7.0, device=cuda) for s in OUT_SHAPES(*shape)]
    gin = [torch.ones(s, device=cuda) for s in OUT_SHAPES(*shape)]
    work = torch.full((B * 15,), 7.0, device=cuda)
    grads = [torch.full_like(x, 7.0) for x in ins[:4]]
    P, stream = _lib.ptr, _lib.stream_ptr(cuda)

    def forward(ins=ins, outs=outs, shape=shape):
        return lib.mr_meshreg_post_forward(*[P(x) for x in ins], *_consts(), *[P(o) for o in outs], *shape, stream)

    def backward(ins=ins, work=work, grads=grads, shape=shape):
        return lib.mr_meshreg_post_backward(*[P(x) for x in ins], *_consts(), *[P(g) for g in gin], P(work), *[P(g) for g in grads],
                                            *shape, stream)

    without = lambda seq, k: [None if i == k else x for i, x in enumerate(seq)]
    for k in range(4):  # a negative count, each of the four
        bad = tuple(-1 if i == k else n for i, n in enumerate(shape))
        assert forward(shape=bad) == MR_ERR_BADARG and backward(shape=bad) == MR_ERR_BADARG
    assert forward(shape=(65536, Vh, J, Vo)) == MR_ERR_BADARG and backward(shape=(65536, Vh, J, Vo)) == MR_ERR_BADARG
    assert forward(ins=without(ins, 4)) == MR_ERR_BADARG and backward(ins=without(ins, 4)) == MR_ERR_BADARG  # a null K
    assert backward(work=None) == MR_ERR_BADARG
    for k in range(5):  # a null output for a non-empty part
        assert forward(outs=without(outs, k)) == MR_ERR_BADARG
    for k in range(4):
        assert backward(grads=without(grads, k)) == MR_ERR_BADARG
    for k in (0, 1, 5):  # a null input for a non-empty part
        assert forward(ins=without(ins, k)) == MR_ERR_BADARG and backward(ins=without(ins, k)) == MR_ERR_BADARG
    assert forward(shape=(0, Vh, J, Vo)) == MR_OK and backward(shape=(0, Vh, J, Vo)) == MR_OK
    torch.cuda.synchronize(cuda)
    for t in outs + grads + [work]:
        assert bool((t == 7.0).all())
    # ... and the accepted call, on the same buffers, overwrites every one of them
    assert forward() == MR_OK and backward() == MR_OK
    torch.cuda.synchronize(cuda)
    for t in outs + grads:
        assert not bool((t == 7.0).any())
