"""The l2 criterion's host side, without a GPU: the routing of a criterion object to its MR_CRITERION_* code, the ABI 9
rows of the ctypes table, the criterion field of the pair-step struct and the plan key that keeps l1 and l2 apart."""
import ctypes

import torch


def test_routing_helper_maps_criteria_to_codes():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
    from handobjectconsist_amd.warping import imgflowarp

    assert imgflowarp._fused_criterion(PyramidCriterion("l1")) == _lib.CRITERION_L1 == 0
    assert imgflowarp._fused_criterion(PyramidCriterion("l2")) == _lib.CRITERION_L2 == 1
    multi = PyramidCriterion("l2")
    multi.level_nb = 2
    assert imgflowarp._fused_criterion(multi) is None
    summed = PyramidCriterion("l1")
    summed.criterion = torch.nn.L1Loss(reduction="sum")
    assert imgflowarp._fused_criterion(summed) is None

    class Foreign:
        level_nb = 1
        criterion = torch.nn.SmoothL1Loss(reduction="none")

    assert imgflowarp._fused_criterion(Foreign()) is None
    assert imgflowarp._fused_criterion(None) is None


def test_abi9_rows_exist_with_the_right_arity():
    from handobjectconsist_amd import _lib

    assert _lib.ABI_VERSION == 9
    for name in ("mr_pair_consist_forward", "mr_pair_consist_backward", "mr_pair_consist_forward_tiles",
                 "mr_pair_consist_backward_tiles", "mr_flow_pair_forward_tiles", "mr_flow_pair_forward_grad_tiles",
                 "mr_flow_pair_backward_tiles"):
        res, args = _lib.SIGNATURES[name + "_crit"]
        old_res, old_args = _lib.SIGNATURES[name]
        assert res is old_res and args == old_args + [ctypes.c_int], name
        assert hasattr(_lib.load(), name + "_crit")


def test_unknown_criterion_is_refused_before_any_device_work():
    from handobjectconsist_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(None)
    # (valid pointers are never looked at: the criterion is checked first)
    assert lib.mr_pair_consist_forward_crit(*([null] * 6), 3, null, 0, *([null] * 11), 1, 8, 8, 0.99999, null, null, 0, null, 7) == -1
    assert lib.mr_flow_pair_backward_tiles_crit(*([null] * 9), 3, *([null] * 8), 8, 8, null, 2, 10, 10, 1, 8, 1e-3, 0.99999, 0, 0,
                                                null, 2) == -1


def test_pair_step_struct_carries_the_criterion():
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    fields = [f for f, _ in pairstep.MrPairStep._fields_]
    assert "criterion" in fields
    assert pairstep.MrPairStep.criterion.offset % 4 == 0
    assert all(getattr(pairstep.MrPairStep, f).offset % 8 == 0 for f, ty in pairstep.MrPairStep._fields_
               if ty in (ctypes.c_void_p, ctypes.c_int64)), "pointers and 64-bit fields naturally aligned"
    lib = _lib.load()
    st = pairstep.MrPairStep()
    for k, v in dict(batch_size=2, num_verts_a=778, num_verts_b=1002, num_hand_faces=1552, num_obj_faces=2000, fill_back=1,
                     image_size=64, height=64, width=64, jitter_channels=3).items():
        setattr(st, k, v)
    sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    for crit, rc in ((_lib.CRITERION_L1, 0), (_lib.CRITERION_L2, 0), (2, -1), (-1, -1)):
        st.criterion = crit
        assert lib.mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == rc, crit


def test_pair_step_plans_are_not_shared_between_criteria(monkeypatch):
    """pair_step keys its plan (struct, scratch) on the criterion: an l1 plan is never reused for an l2 call of the same
    shape.  The device call itself is replaced (no GPU here): what is checked is the plan selection and the struct field."""
    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import pairstep

    seen = []

    def fake_apply(h1, o1, h2, o2, call):
        plan = call[0]
        seen.append((plan, int(plan.st.criterion)))
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
    img, jit = torch.zeros(B, 3, H, H), torch.ones(B, 3, H, H)
    for crit in (_lib.CRITERION_L1, _lib.CRITERION_L2, _lib.CRITERION_L1):
        try:
            pairstep.pair_step((h1, o1), (h1, o1), hf, of, K, K, Ren(), 64, H, H, img, img, jit, jit, None, criterion=crit)
        except StopIteration:
            pass
    (p1, c1), (p2, c2), (p3, c3) = seen
    assert (c1, c2, c3) == (0, 1, 0)
    assert p1 is not p2 and p1 is p3, "an l1 plan must never serve an l2 call (and is reused for l1)"
