"""tests/pair_upstream_cases.py on the CPU: what tests/test_gpu_pair_upstream.py relies on, proven without a device.

Upstream specs.  Every per-sample coefficient of every spec, at every batch size the spec is used at, is the same fp32 number in
every order of fp32 additions of its terms and equals their float64 sum: the device (``gl_dir + gl_sum + gl_mean / B``), torch's
autograd on the node path and the oracle add in orders of their own, and none of them rounds.  The oracle's gradient for a
spec is a combination of two unit results (``pair_oracle_harness.oracle_units``); at the default weights it is compared with the
one-chain oracle the older tests use.  Bound of that comparison: the chains differ in where the coefficient meets the fp32
per-pixel gradient of ``W.pair_consist_grad`` -- one fp32 rounding of ``coefficient / count`` and one of its product per pixel,
2^-23 relative per term, summed in float64 -- so 1e-6 of the sample's largest gradient (a tenth of the rule's absolute term,
some eight times 2^-23) bounds it with room for cancellation between a vertex's pixels.

Headroom.  tests/host/launch_plan_cases.cpp (``scatter``) calls the functions of csrc/launch_plan.hpp with which
``unit_scatter_tiles_kernel`` hands an image's covered tiles to workgroups and forms ``terms`` / ``headroom`` in front of its
second pass (``st_parts``, ``st_second_q``, ``st_used``, ``st_share``, ``st_terms``, ``st_headroom``), on that header's own plan.
Fed with the oracle's coverage it proves that X1 (raster 132) reaches headroom 1 and X2 (raster 196) headroom 2 in every
workgroup, for both seeds, that the next smaller rasters the fused path accepts (128, 192) reach one less even when every tile
is covered, and that NO case of tests/pair_mesh_cases.py, tests/pair_border_cases.py nor the 1 x 480 shape of
tests/test_gpu_compact_batch.py reaches headroom 1: before these cases the suite never ran the scatter with a reduced shift.
(Rasters of at most 64 tiles -- 128 x 128 and below -- cannot: whatever is covered, one tile per wave fits the grid, q stays 8.)
"""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

from handobjectconsist_amd.utils import synth
from oracle import raster_ref as R
from oracle import warp_ref as W
from tests import pair_border_cases as PB
from tests import pair_mesh_cases as P
from tests import pair_oracle_harness as H
from tests import pair_upstream_cases as PU
from tests.test_launch_plan_host import _host_compiler
from tests.test_pair_mesh_cases_host import SOURCE

SPEC_AT = [(k, B) for k in PU.SPECS for B in PU.USED_AT[k]]


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("name,B", SPEC_AT)
def test_every_coefficient_is_exact_in_every_order(name, B):
    spec = PU.SPECS[name](B)
    ups = [spec] + ([spec.scaled(PU.LOSS_SCALE)] if name.startswith("all/") else [])
    for up in ups:
        if up.wm is not None:
            assert np.float64(np.float32(up.wm) / np.float32(B)) == np.float64(up.wm) / B, "the mean's share must be exact in fp32"
        cf, cb = up.coefficients(B) if name not in ("inf", "nan") else (None, None)
        for which, per_sample in zip("fb", up.terms(B)):
            for b, terms in enumerate(per_sample):
                with np.errstate(invalid="ignore"):
                    exact = sum((np.float64(t) for t in terms), np.float64(0))
                    for order in itertools.permutations(terms):
                        acc = np.float32(0) if not order else order[0]
                        for t in order[1:]:
                            acc = np.float32(acc + t)
                        assert _same(np.float64(acc), exact), (name, B, which, b, order)
                if cf is not None:
                    assert exact == (cf if which == "f" else cb)[b]
    # what the spec is for
    for b in PU.ZERO_GRAD_SAMPLES.get(name, ()):
        cf, cb = spec.coefficients(B)
        assert b >= B or (cf[b] == 0 and cb[b] == 0)
    if name == "cancel":
        tf, tb = spec.terms(B)
        assert all(t != 0 for t in tf[1] + tb[1] + tb[3]) and spec.coefficients(B)[1][3] == 0 and spec.coefficients(B)[0][3] != 0
    if name == "denormal":
        tiny = np.float32(spec.wf[1])
        assert 0 < tiny < np.finfo(np.float32).tiny and float(tiny) == 2.0 ** -140 and spec.wb[1] == tiny
    if name == "spread" and B == 4:
        mags = np.abs(np.concatenate([spec.wf, spec.wb]))
        assert mags.max() >= 2.0 ** 100 and mags[mags > 0].min() <= 2.0 ** -99 and (spec.wf < 0).any() and (spec.wf > 0).any()
    if name == "mean/fwd":
        assert not spec.coefficients(B)[1].any() and spec.coefficients(B)[0].all()


@pytest.mark.parametrize("name", ["W1", "I"])
def test_the_unit_combination_is_the_one_chain_oracle(name):
    case = H.CASES[name]
    seed, B = case["seed"], case["B"]
    direct = H.oracle(name, seed)["grads"]
    combined = H.oracle(name, seed, upstream=H.default_upstream(B))["grads"]
    for d, c, leaf in zip(direct, combined, H.LEAVES):
        scale = np.abs(d).max(axis=(1, 2), keepdims=True)
        assert scale.min() > 0
        worst = float((np.abs(d - c) / scale).max())
        print(f"{name} d/d {leaf}: combination against the one-chain oracle: {worst:.2e} of the sample's largest gradient")
        assert worst <= 1e-6, (name, leaf, worst)
    # (the default weights, for the record, are NOT exact in fp32 -- linspace's thirds -- which is why they are not a spec)
    cf, cb = H.default_upstream(B).coefficients(B)
    wf, wb, ws = H.weights(B)
    assert np.allclose(cf, wf.astype(np.float64) + ws + H.WM / B, rtol=1e-6) and np.allclose(cb, wb.astype(np.float64) + ws + H.WM / B, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------
# headroom
# ---------------------------------------------------------------------------------------------------


def _tiles(raster):
    return ((raster + 7) // 8) * ((raster + 31) // 32)


def _rows():
    """name -> (B2, V, raster, counts of covered tiles per image, how the counts were got)"""
    rows = {}
    for name, case in PU.CASES.items():
        for d in (0, H.SECOND_SEED):
            B2, V, _, _, _, is_ = P.plan_row(case)
            rows[f"{name}/{case['seed'] + d}"] = (B2, V, is_, PU.covered_tiles(H.oracle_forward(name, case["seed"] + d), is_), "oracle")
        # the next smaller raster the fused path accepts, with every tile covered
        rows[f"{name}/below"] = (B2, V, is_ - 4, [_tiles(is_ - 4)] * B2, "all tiles")
    for name, case in {**P.CASES, **PB.CASES}.items():
        if not case["fused"]:
            continue  # (K, L: the composed path, no unit scatter)
        B2, V, _, _, _, is_ = P.plan_row(case)
        if _tiles(is_) <= 64:
            rows[name] = (B2, V, is_, [_tiles(is_)] * B2, "all tiles")
        else:
            for d in (0, H.SECOND_SEED):
                rows[f"{name}/{case['seed'] + d}"] = (B2, V, is_, PU.covered_tiles(H.oracle_forward(name, case["seed"] + d), is_), "oracle")
    # the 1 x 480 shape of tests/test_gpu_compact_batch.py: synth.random_scene at that test's seed (41 + B)
    e = P.EXISTING_480
    s = synth.random_scene(e["B"], seed=41 + e["B"], image_size=e["raster"])
    kw = dict(R=np.eye(3, dtype=np.float32)[None], t=np.zeros((1, 3), np.float32), dist_coeffs=np.zeros((1, 5), np.float32), orig_size=e["raster"],
              image_size=e["raster"], anti_aliasing=False, near=0.1, far=100, eps=1e-3, num_threads=8, keep_saved=True)
    _, renders, _ = W.get_opticalflow(R, [s["verts1"], s["verts2"]], s["faces"], [s["K1"], s["K2"]], kw, orig_img_size=(e["raster"], e["raster"]),
                                      ignore_face_idxs=synth.HAND_IGNORE_FACES, return_renders=True, return_masks=True)
    rows["480"] = (2 * e["B"], s["verts1"].shape[1], e["raster"], PU.covered_tiles(dict(renders=renders), e["raster"]), "oracle")
    return rows


@pytest.fixture(scope="module")
def scatter(tmp_path_factory):
    """row name -> ({field: value}, the row)"""
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_cases")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SOURCE], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    rows = _rows()
    text = "".join(f"{B2} {V} {is_} " + " ".join(str(n) for n in counts) + "\n" for B2, V, is_, counts, _ in rows.values())
    run = subprocess.run([exe, "scatter"], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows), run.stdout
    out = {}
    for (name, row), line in zip(rows.items(), lines):
        d = dict(item.split("=") for item in line.split())
        assert int(d["status"]) == 0, (name, line)
        d["wgs"] = [tuple(int(x) for x in w.split(".")) for w in d["wgs"].split(";")]  # (image, tiles, terms, headroom)
        print(f"{name} ({row[4]}): raster {row[2]}, covered tiles {sorted(set(row[3]))} of {_tiles(row[2])}, groups {d['groups']}, q {d['q']}, "
              f"workgroups per image {sorted(set(d['per_image'].split(',')))}, tiles per workgroup {sorted({w[1] for w in d['wgs']})}, headroom {sorted({w[3] for w in d['wgs']})}")
        out[name] = (d, row)
    return out


@pytest.mark.parametrize("name", list(PU.CASES))
def test_the_new_cases_reach_their_headroom_and_are_the_smallest(scatter, name):
    want = PU.HEADROOM[name]
    case = PU.CASES[name]
    assert case["raster"] <= 320 and case["raster"] % 4 == 0 and case["B"] in (1, 2)
    for seed in (case["seed"], case["seed"] + H.SECOND_SEED):
        d, row = scatter[f"{name}/{seed}"]
        assert int(d["max_headroom"]) == want, (name, seed, d)
        # (every image has a workgroup at that headroom: both directions and every sample are summed with the reduced shift)
        assert {w[0] for w in d["wgs"] if w[3] == want} == set(range(row[0])), (name, seed, d["wgs"])
        # the three lines, once more in Python: terms = 3 x 32 x 8 per tile (one tile per wave and round), 2^13 per bit
        for _, tiles, terms, headroom in d["wgs"]:
            assert terms == 768 * tiles and (terms >> headroom) < 8192 and (headroom == 0 or (terms >> (headroom - 1)) >= 8192)
    d, _ = scatter[f"{name}/below"]
    assert int(d["max_headroom"]) == want - 1, f"raster {case['raster'] - 4} already reaches headroom {want}: move {name} down"


def test_no_older_case_reaches_headroom_1(scatter):
    older = {n: v for n, v in scatter.items() if n.split("/")[0] not in PU.CASES}
    assert {n.split("/")[0] for n in older} == {n for n, c in {**P.CASES, **PB.CASES}.items() if c["fused"]} | {"480"}
    reached = {n: int(d["max_headroom"]) for n, (d, _) in older.items() if int(d["max_headroom"]) >= 1}
    assert not reached, f"cases that already ran the scatter with a reduced shift: {reached}"
    assert int(scatter["480"][0]["groups"]) == 32 and int(scatter["H/8"][0]["groups"]) == 16


@pytest.mark.parametrize("name", list(PU.CASES))
def test_the_fused_path_takes_the_new_cases(name):
    import types

    from handobjectconsist_amd import _lib
    from handobjectconsist_amd.warping import opticalflow, pairstep

    case = PU.CASES[name]
    B2, V, Fh, Fo, _, is_ = P.plan_row(case)
    s = PB.wall_scene(case)
    assert s["hand_faces"].max() < synth.HAND_VERTS and s["obj_faces"].max() < case["obj_verts"] and V <= 2560
    assert min(s["verts1"][..., 2].min(), s["verts2"][..., 2].min()) > 0.2
    assert opticalflow._stacked_flow_node_ok(types.SimpleNamespace(image_size=is_, anti_aliasing=False), V)
    st = pairstep.MrPairStep()
    sizes = dict(batch_size=case["B"], num_verts_a=synth.HAND_VERTS, num_verts_b=V - synth.HAND_VERTS, num_hand_faces=Fh, num_obj_faces=Fo,
                 fill_back=1, image_size=is_, height=case["crop"][1], width=case["crop"][0], jitter_channels=case["jitter_channels"])
    for k, v in sizes.items():
        setattr(st, k, v)
    sc, sv, th = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert _lib.load().mr_pair_step_sizes(ctypes.byref(st), ctypes.byref(sc), ctypes.byref(sv), ctypes.byref(th)) == 0
