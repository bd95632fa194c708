"""Randomised parity sweeps of the HIP path against the CPU oracle (not collected by pytest: a bug hunt to run
on the GPU box).  Usage: python tests/fuzz_parity.py [n_cases] [first_seed]  (HOC_FUZZ_RASTER_ONLY=1: the first sweep
alone; HOC_FUZZ_DEBUG=1: details of non-finite gradients).  Found the NaN-depth point-face bug
and the collinear-face bounding-box bug, in round 4 that kernel D's strip bookkeeping refused rasters of one or two pixels;
30 000+ cases clean since (the final build of round 4: 2 500 + 2 500 + 300 ... cases of seed 960000 on, all eight sweeps)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from handobjectconsist_amd.neurender import rasterize
from handobjectconsist_amd.warping import imgflowarp
from handobjectconsist_amd.optim.pyramidloss import PyramidCriterion
from handobjectconsist_amd.utils import synth
from oracle import raster_ref as R, warp_ref as W

dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)
n_cases, seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 0
KW = dict(R=np.eye(3, dtype=np.float32)[None], t=np.zeros((1, 3), np.float32), dist_coeffs=np.zeros((1, 5), np.float32))
bad = 0
COVER = {}
t0 = time.time()
for case in range(n_cases):
    seed = seed0 + case
    rng = np.random.default_rng(seed)
    B, is_ = int(rng.integers(1, 4)), int(rng.integers(9, 161))
    kind = ("scene", "big", "tiny", "degenerate", "collinear")[int(rng.integers(0, 5))]
    if kind == "scene":
        s = synth.random_scene(B, seed=seed, image_size=is_)
        cols = rng.uniform(-2, 2, (B, s["verts1"].shape[1], 3)).astype(np.float32)
        f2, tex = R.fill_back(s["faces"], R.batch_vertex_textures(s["faces"], cols))
        faces = R.nr_vertices_to_faces(R.nr_projection(s["verts1"], s["K1"], KW["R"], KW["t"], KW["dist_coeffs"], is_), f2)
    else:
        n = int(rng.integers(1, 60))
        faces = rng.uniform(-1.4, 1.4, (B, n, 3, 3)).astype(np.float32)
        if kind == "tiny":
            faces[..., :2] = faces[:, :, :1, :2] + rng.uniform(-0.03, 0.03, (B, n, 3, 2)).astype(np.float32)
        faces[..., 2] = rng.uniform(0.05, 3.0, (B, n, 3))
        if kind == "collinear":  # vertices p + k * d with exactly representable steps, optionally nudged by one ulp
            p0 = np.round(rng.uniform(-1, 1, (B, n, 1, 2)) * 64) / 64
            d = np.round(rng.uniform(-1, 1, (B, n, 1, 2)) * 32) / 32 * 2.0 ** rng.integers(-3, 6, (B, n, 1, 1))
            k = rng.integers(-3, 4, (B, n, 3, 1)).astype(np.float32)
            faces[..., :2] = (p0 + k * d).astype(np.float32)
            nudge = rng.random((B, n, 3, 2)) < 0.15
            faces[..., :2] = np.where(nudge, np.nextafter(faces[..., :2], np.float32(np.inf)), faces[..., :2])
        if kind == "degenerate":
            faces[:, ::3, 2] = faces[:, ::3, 0]                       # zero area
            faces[:, 1::5, 1, :2] = faces[:, 1::5, 0, :2]             # repeated vertex
            faces[:, 2::7, :, 0] = faces[:, 2::7, :1, 0]              # vertical line
            faces = np.round(faces * 8) / 8 if rng.random() < 0.5 else faces  # vertices on pixel-centre lattices
        if rng.random() < 0.15:
            faces[..., :2] *= (5.0, 50.0, 1e4)[int(rng.integers(0, 3))]   # far off-screen vertices, huge bboxes
        if rng.random() < 0.2:  # vertices at / behind / absurdly far from the camera plane
            special = np.array([0.0, -1.0, 1e-20, 1e20, np.inf, -0.0, 0.1, 100.0], np.float32)
            hit = rng.random(faces.shape[:3]) < 0.15
            faces[..., 2] = np.where(hit, special[rng.integers(0, len(special), faces.shape[:3])], faces[..., 2])
        faces = np.ascontiguousarray(np.concatenate([faces, faces[:, :, ::-1]], 1))
        ts = (2, 2, 2, 3, 4)[int(rng.integers(0, 5))]
        tex = rng.uniform(-1, 1, (B, faces.shape[1], ts, ts, ts, 3)).astype(np.float32)
    if rng.random() < 0.1 and kind != "scene":
        is_ = int(rng.integers(250, 330))
    elif rng.random() < 0.08:
        is_ = int(rng.integers(1, 9))
    near, far = (0.1, 100.0) if rng.random() < 0.6 else (float(rng.uniform(0.05, 1.0)), float(rng.uniform(1.2, 3.5)))
    eps = (1e-3, 1e-3, 1e-4, 1e-2, 1e-6, 0.3)[int(rng.integers(0, 6))]
    ref = R.rasterize_rgbad(faces, tex, is_, False, near, far, eps, (0.1, 0.2, 0.3), num_threads=8, keep_saved=True)
    f_t, x_t = t(faces).requires_grad_(True), t(tex).requires_grad_(True)
    out = rasterize.rasterize_rgbad(f_t, x_t, is_, False, near, far, eps, (0.1, 0.2, 0.3))
    msg = []
    COVER.setdefault(kind, []).append(float((ref["face_index_map"] >= 0).mean()))
    nf = int((out["face_index_map"].cpu().numpy() != ref["face_index_map"]).sum())
    if nf: msg.append(f"face_index_map differs at {nf} px")
    for k, tol in (("rgb", 1e-5), ("depth", 1e-6), ("alpha", 0)):
        e = np.abs(out[k].detach().cpu().numpy().astype(np.float64) - ref[k]).max()
        if e > tol * max(1.0, np.abs(ref[k]).max()): msg.append(f"{k} err {e:.2e}")
    saved = ref["_saved"]
    g = [rng.standard_normal(saved[k].shape).astype(np.float32) for k in ("rgb_map", "alpha_map", "depth_map")]
    gf_ref, gt_ref = R.rasterize_backward(saved, *g, num_threads=8)
    img = [np.ascontiguousarray(g[0].transpose(0, 3, 1, 2)[:, :, ::-1]), np.ascontiguousarray(g[1][:, ::-1]), np.ascontiguousarray(g[2][:, ::-1])]
    torch.autograd.backward([out["rgb"], out["alpha"], out["depth"]], [t(a) for a in img])
    for got, want, name in ((x_t.grad, gt_ref, "grad_textures"), (f_t.grad, gf_ref, "grad_faces")):
        gotn = got.cpu().numpy().astype(np.float64)
        if not np.isfinite(gotn).all() and np.isfinite(want).all():
            msg.append(f"{name} non-finite")
            if os.environ.get("HOC_FUZZ_DEBUG"):  # which rows, and does the ordered walk (MR_FLAG_REFERENCE_ALGO) agree with the oracle?
                rows = np.argwhere(~np.isfinite(gotn).reshape(gotn.shape[0], gotn.shape[1], -1).all(-1))
                print("   non-finite rows (image, face):", rows[:6].tolist(), "eps", eps, "near/far", near, far)
                for bi, fi in rows[:3]:
                    print("   face", faces[bi, fi].tolist(), "\n   got", gotn[bi, fi].reshape(-1).tolist(), "\n   want", np.asarray(want)[bi, fi].reshape(-1).tolist())
                rasterize.REFERENCE_ALGO = True
                try:
                    f_r, x_r = t(faces).requires_grad_(True), t(tex).requires_grad_(True)
                    o_r = rasterize.rasterize_rgbad(f_r, x_r, is_, False, near, far, eps, (0.1, 0.2, 0.3))
                    torch.autograd.backward([o_r["rgb"], o_r["alpha"], o_r["depth"]], [t(a) for a in img])
                    print("   ordered walk finite:", bool(torch.isfinite(f_r.grad).all()), bool(torch.isfinite(x_r.grad).all()))
                finally:
                    rasterize.REFERENCE_ALGO = False
        sc = np.abs(want[np.isfinite(want)]).max() if np.isfinite(want).any() else 1.0
        e = np.abs(np.nan_to_num(gotn - want)).max()
        # absolute floor: a face covering the whole image sums is^2 unit-variance terms that largely cancel; the fp32
        # rounding of that sum (sequential in the oracle, tree / atomic order on the GPU) is ~1e-6 * sqrt(is^2) whatever
        # the size of the result (seed 201795: depth backward of a 1e4-NDC face over 62 x 62 px, 3.7e-5 on 0.063)
        if e > 2e-4 * sc + 1e-6 * max(is_, 1): msg.append(f"{name} err {e:.2e} (scale {sc:.2e})")
    if case % 4 == 1:  # silhouette / depth entry points (module-default eps) and the anti-aliased render
        aa = bool(rng.random() < 0.5)
        sil = rasterize.rasterize_silhouettes(t(faces), is_, aa).cpu().numpy()
        dep = rasterize.rasterize_depth(t(faces), is_, aa).cpu().numpy()
        r2 = R.rasterize_rgbad(faces, None, is_, aa, 0.1, 100, 1e-4, None, False, True, True, num_threads=8)
        if np.abs(sil - r2["alpha"]).max() > 1e-6: msg.append("silhouette mode")
        dd = np.abs(dep - r2["depth"]); dd = dd[np.isfinite(dd)]
        if dd.size and dd.max() > 1e-5 * max(1.0, float(np.abs(r2["depth"][np.isfinite(r2["depth"])]).max())): msg.append(f"depth mode err {dd.max():.2e}")
        if kind == "scene" or ts == 2:
            f5, x5 = t(faces).requires_grad_(True), t(tex).requires_grad_(True)
            o5 = rasterize.rasterize_rgbad(f5, x5, is_, True, near, far, eps, (0.1, 0.2, 0.3))
            r5 = R.rasterize_rgbad(faces, tex, is_, True, near, far, eps, (0.1, 0.2, 0.3), num_threads=8, keep_saved=True)
            # backward through the 2 x 2 average pooling: image gradients spread over the 2x raster, / 4
            gi = [rng.standard_normal((B, 3, is_, is_)).astype(np.float32), rng.standard_normal((B, is_, is_)).astype(np.float32),
                  rng.standard_normal((B, is_, is_)).astype(np.float32)]
            torch.autograd.backward([o5["rgb"], o5["alpha"], o5["depth"]], [t(a) for a in gi])
            up = lambda a: np.repeat(np.repeat(a, 2, -1), 2, -2) / np.float32(4)
            g2 = [np.ascontiguousarray(up(gi[0])[:, :, ::-1].transpose(0, 2, 3, 1)), np.ascontiguousarray(up(gi[1])[:, ::-1]),
                  np.ascontiguousarray(up(gi[2])[:, ::-1])]
            gf5, gt5 = R.rasterize_backward(r5["_saved"], *g2, num_threads=8)
            for got, want, name in ((x5.grad, gt5, "aa grad_textures"), (f5.grad, gf5, "aa grad_faces")):
                sc = np.abs(want[np.isfinite(want)]).max() if np.isfinite(want).any() else 1.0
                e = np.abs(np.nan_to_num(got.cpu().numpy().astype(np.float64) - want)).max()
                if e > 5e-4 * sc + 1e-6:  # (1e7-scale pseudo-gradients of degenerate faces)
                    msg.append(f"{name} err {e:.2e} (scale {sc:.2e})")
            if (o5["face_index_map"].cpu().numpy() != r5["face_index_map"]).any(): msg.append("aa fim")
            e5 = np.abs(o5["rgb"].detach().cpu().numpy() - r5["rgb"]); e5 = e5[np.isfinite(e5)]
            if e5.size and e5.max() > 1e-5 * max(1.0, float(np.abs(r5["rgb"][np.isfinite(r5["rgb"])]).max())): msg.append(f"aa rgb err {e5.max():.2e}")
    if case % 3 == 0:  # the upstream-compatible five-entry-point path and the reference-algorithm kernels
        f3, x3 = t(faces).requires_grad_(True), t(tex).requires_grad_(True)
        rgb3, alpha3, depth3, fim3, finv3, wmap3 = rasterize.RasterizeFunction.apply(f3, x3, is_, near, far, eps, (0.1, 0.2, 0.3), True, True, True)
        if (fim3.cpu().numpy() != saved["face_index_map"]).any(): msg.append("compat fim")
        if np.abs(rgb3.detach().cpu().numpy() - saved["rgb_map"]).max() > 1e-5: msg.append("compat rgb")
        torch.autograd.backward([rgb3, alpha3, depth3], [t(a) for a in g])
        for got, want, name in ((x3.grad, gt_ref, "compat grad_textures"), (f3.grad, gf_ref, "compat grad_faces")):
            sc = np.abs(want[np.isfinite(want)]).max() if np.isfinite(want).any() else 1.0
            e = np.abs(np.nan_to_num(got.cpu().numpy().astype(np.float64) - want)).max()
            if e > 2e-4 * sc + 1e-6 * max(is_, 1): msg.append(f"{name} err {e:.2e} (scale {sc:.2e})")
        rasterize.REFERENCE_ALGO = True
        try:
            f4, x4 = t(faces).requires_grad_(True), t(tex).requires_grad_(True)
            o4 = rasterize.rasterize_rgbad(f4, x4, is_, False, near, far, eps, (0.1, 0.2, 0.3))
            if (o4["face_index_map"].cpu().numpy() != ref["face_index_map"]).any(): msg.append("reference-algo fim")
            torch.autograd.backward([o4["rgb"], o4["alpha"], o4["depth"]], [t(a) for a in img])
            sc = np.abs(gf_ref[np.isfinite(gf_ref)]).max() if np.isfinite(gf_ref).any() else 1.0
            e = np.abs(np.nan_to_num(f4.grad.cpu().numpy().astype(np.float64) - gf_ref)).max()
            if e > 2e-4 * sc + 1e-6 * max(is_, 1): msg.append(f"reference-algo grad_faces err {e:.2e} (scale {sc:.2e})")
        finally:
            rasterize.REFERENCE_ALGO = False
    # warp half: random flows incl. out-of-range and exactly integer ones
    H, Wd = int(rng.integers(1, 70)), int(rng.integers(1, 90))
    fl = [rng.normal(0, 3, (B, H, Wd, 2)).astype(np.float32) for _ in range(2)]
    for f in fl:
        f[rng.random(f.shape[:3]) < 0.2] = 0
        f[rng.random(f.shape[:3]) < 0.1] = np.round(f[rng.random(f.shape[:3]) < 0.1][: 0].sum() + 2.0)
    im = [rng.uniform(-0.5, 0.5, (B, 3, H, Wd)).astype(np.float32) for _ in range(2)]
    jm = [np.ones((B, 3, H, Wd), np.float32) for _ in range(2)]
    for m in jm:
        m[:, :, : int(rng.integers(0, 3))] = 0
    ub = bool(rng.random() < 0.7)
    ref_loss = W.pair_consist(fl, im[0], im[1], jm[0], jm[1], ub)[0]
    fl_t = [t(fl[0]).requires_grad_(True), t(fl[1]).requires_grad_(True)]
    loss = imgflowarp.pair_consist(fl_t, t(im[0]), t(im[1]), t(jm[0]), t(jm[1]), PyramidCriterion("l1"), use_backward=ub, outputs="loss")[0]
    e = np.abs(loss.detach().cpu().numpy() - ref_loss).max()
    if e > 1e-5 * max(1.0, np.abs(ref_loss).max()): msg.append(f"pair loss err {e:.2e}")
    gl = rng.standard_normal(B).astype(np.float32)
    ref_gf = W.pair_consist_grad(fl, im[0], im[1], jm[0], jm[1], gl, ub)
    (loss * t(gl)).sum().backward()
    for i in (0, 1):
        got = fl_t[i].grad.cpu().numpy() if fl_t[i].grad is not None else np.zeros_like(ref_gf[i])
        e, sc = np.abs(got - ref_gf[i]).max(), np.abs(ref_gf[i]).max() + 1e-12
        if e > 1e-4 * sc + 1e-9: msg.append(f"grad_flow{i} err {e:.2e} (scale {sc:.2e})")
    if msg:
        bad += 1
        print(f"seed {seed} {kind} B={B} is={is_} F={faces.shape[1]}: " + "; ".join(msg))
print(f"{n_cases} cases, {bad} with mismatches, {time.time() - t0:.0f} s; mean covered fraction by kind:",
      {k: round(float(np.mean(v)), 3) for k, v in COVER.items()})

if os.environ.get("HOC_FUZZ_RASTER_ONLY"):  # (a long run of the first sweep alone)
    sys.exit(1 if bad else 0)

# ---- second sweep: vertex-colour path (indexed meshes, shared vertices, degenerate triangles), compat API,
# ---- reference-algorithm flag, anti-aliasing, warp / occlusion kernels
from handobjectconsist_amd.neurender.renderer import Renderer
bad2 = 0
t0 = time.time()
for case in range(n_cases):
    seed = seed0 + 100000 + case
    rng = np.random.default_rng(seed)
    B, is_ = int(rng.integers(1, 4)), int(rng.integers(8, 140))
    V, F0 = int(rng.integers(3, 80)), int(rng.integers(1, 120))
    verts = rng.uniform(-0.25, 0.25, (B, V, 3)).astype(np.float32)
    verts[..., 2] = rng.uniform(0.3, 0.9, (B, V))
    if rng.random() < 0.3:
        verts[:, : V // 3] = verts[:, :1]  # coincident vertices -> zero-area / point faces
    fidx = rng.integers(0, V, (B, F0, 3)).astype(np.int64)  # may repeat a vertex within a face
    f = float(rng.uniform(100, 400)) * is_ / 256
    K = np.tile(np.array([[f, 0, is_ / 2], [0, f, is_ / 2], [0, 0, 1]], np.float32), (B, 1, 1))
    cols = rng.uniform(-2, 2, (B, V, 3)).astype(np.float32)
    aa, fb = bool(rng.random() < 0.3), bool(rng.random() < 0.7)
    msg = []
    ren = Renderer(image_size=is_, R=torch.eye(3, device=dev)[None], t=torch.zeros(1, 3, device=dev), K=torch.ones(1, 3, 3, device=dev),
                   orig_size=is_, anti_aliasing=aa, fill_back=fb, near=0.1, no_light=True)
    c1 = t(cols).requires_grad_(True)
    # the SAME projected vertices on both sides (numpy projection): the rasterisers must then agree exactly
    v_ndc = R.nr_projection(verts, K, KW["R"], KW["t"], KW["dist_coeffs"], is_)
    out = ren.render_projected_vertex_colors(t(v_ndc), t(fidx), c1)
    tex = R.batch_vertex_textures(fidx, cols)
    f2, tex2 = R.fill_back(fidx, tex) if fb else (fidx, tex)
    ref = R.rasterize_rgbad(R.nr_vertices_to_faces(v_ndc, f2), tex2, is_, aa, 0.1, 100, 1e-3, (0, 0, 0), num_threads=8)
    a, b = out["face_index_map"].cpu().numpy(), ref["face_index_map"]
    nd = int((a != b).sum())
    if nd: msg.append(f"vc fim differs at {nd} px")
    same = (a == b)
    if aa:
        pass
    else:
        e = np.abs(out["rgb"].detach().cpu().numpy() - ref["rgb"])[np.broadcast_to(same[:, None, ::-1], ref["rgb"].shape)].max() if same.any() else 0
        if e > 2e-3: msg.append(f"vc rgb err {e:.2e}")
    g = torch.randn_like(out["rgb"])
    out["rgb"].backward(g)
    c2 = t(cols).requires_grad_(True)
    from handobjectconsist_amd.utils import textutils
    out2 = ren(t(verts), t(fidx), textutils.batch_vertex_textures(t(fidx), c2), K=t(K), detach_renders=True)
    out1 = ren.render_vertex_colors(t(verts), t(fidx), c1.detach(), K=t(K))  # same (GPU) projection as out2
    if not torch.equal(out2["face_index_map"], out1["face_index_map"]) or not torch.equal(out2["rgb"], out1["rgb"]): msg.append("vc != generic forward")
    if not torch.equal(out2["face_index_map"], out["face_index_map"]):
        c1.grad = None  # projections differ in the last bit on this case: compare the gradients on the GPU projection
        c1g = c1.detach().clone().requires_grad_(True)
        out = ren.render_vertex_colors(t(verts), t(fidx), c1g, K=t(K))
        out["rgb"].backward(g)
        c1 = c1g
    out2["rgb"].backward(g)
    e = float((c1.grad - c2.grad).abs().max()); sc = float(c2.grad.abs().max()) + 1e-12
    if e > 2e-4 * sc: msg.append(f"vc grad vs generic err {e:.2e} (scale {sc:.2e})")
    # warp + occlusion kernels
    H, Wd = int(rng.integers(1, 50)), int(rng.integers(1, 60))
    x = rng.standard_normal((B, 3, H, Wd)).astype(np.float32)
    fl = rng.normal(0, 4, (B, 2, H, Wd)).astype(np.float32)
    fl[rng.random(fl.shape) < 0.15] = np.round(fl[rng.random(fl.shape) < 0.15][:0].sum() + 1.0)
    for mode in ("bilinear", "nearest"):
        ro, rm = W.warp(x, fl, mode=mode)
        xt, ft = t(x).requires_grad_(True), t(fl).requires_grad_(True)
        go, gm = imgflowarp.warp(xt, ft, mode=mode)
        if np.abs(go.detach().cpu().numpy() - ro).max() > 1e-5 or (gm.cpu().numpy() != rm).any(): msg.append(f"warp {mode}")
        if mode == "bilinear":
            gout = rng.standard_normal(x.shape).astype(np.float32)
            rgf, rgx = W.warp_backward(x, fl, gout)
            go.backward(t(gout))
            for got, want, name in ((ft.grad, rgf, "warp grad_flow"), (xt.grad, rgx, "warp grad_x")):
                e, sc = np.abs(got.cpu().numpy() - want).max(), np.abs(want).max() + 1e-12
                if e > 1e-4 * sc + 1e-6: msg.append(f"{name} err {e:.2e} (scale {sc:.2e})")
    m1, m2 = (rng.random((B, 1, H, Wd)) < 0.7).astype(np.float32), (rng.random((B, 1, H, Wd)) < 0.7).astype(np.float32)
    f12 = np.concatenate([rng.normal(0, 3, (B, 2, H, Wd)), np.ones((B, 1, H, Wd))], 1).astype(np.float32) * m1
    f21 = np.concatenate([rng.normal(0, 3, (B, 2, H, Wd)), np.ones((B, 1, H, Wd))], 1).astype(np.float32) * m2
    if H > 1 and Wd > 1:
        r1, r2 = W.get_occlusion_mask(m1, m2, f12, f21)
        g1, g2 = imgflowarp.get_occlusion_mask(t(m1), t(m2), t(f12), t(f21))
        if (g1.cpu().numpy() != r1).any() or (g2.cpu().numpy() != r2).any(): msg.append("occlusion mask")
    if msg:
        bad2 += 1
        print(f"seed {seed} B={B} is={is_} V={V} F0={F0} aa={aa} fb={fb} HxW={H}x{Wd}: " + "; ".join(msg))
print(f"sweep 2: {n_cases} cases, {bad2} with mismatches, {time.time() - t0:.0f} s")

# ---- third sweep: MANO LBS kernels vs the PyTorch restatement (pose magnitudes from ~0 to several radians)
from handobjectconsist_amd.models import synthnet
layer = synthnet.SynthManoLayer(ncomps=15, use_pca=True, center_idx=9).to(dev)
bad3 = 0
for case in range(min(n_cases, 300)):
    seed = seed0 + 200000 + case
    g = torch.Generator().manual_seed(seed)
    B = int(torch.randint(1, 70, (1,), generator=g))
    scale = float(10 ** torch.empty(1).uniform_(-6, 0.7, generator=g))
    pose = (scale * torch.randn(B, 18, generator=g)).to(dev)
    beta = (3 * torch.randn(B, 10, generator=g)).to(dev)
    p1, b1 = pose.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    p2, b2 = pose.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    v1, j1 = layer(p1, b1)
    v2, j2 = layer.forward_torch(p2, b2)
    wv, wj = torch.randn(v2.shape, generator=g).to(dev), torch.randn(j2.shape, generator=g).to(dev)
    ((v1 * wv).sum() + (j1 * wj).sum()).backward()
    ((v2 * wv).sum() + (j2 * wj).sum()).backward()
    sc = float(v2.detach().abs().max())
    msg = []
    dv, dj = float((v1 - v2).detach().abs().max()), float((j1 - j2).detach().abs().max())
    if dv > 2e-5 * sc: msg.append(f"verts err {dv:.2e}")
    if dj > 2e-5 * sc: msg.append(f"joints err {dj:.2e}")
    for a, b_, name in ((p1.grad, p2.grad, "grad pose"), (b1.grad, b2.grad, "grad betas")):
        e, s_ = float((a - b_).abs().max()), float(b_.abs().max()) + 1e-12
        if not torch.isfinite(a).all() or e > 3e-4 * s_: msg.append(f"{name} err {e:.2e} (scale {s_:.2e})")
    if msg:
        bad3 += 1
        print(f"seed {seed} B={B} pose scale {scale:.1e}: " + "; ".join(msg))
print(f"sweep 3 (MANO): {min(n_cases, 300)} cases, {bad3} with mismatches")

# ---- fourth sweep: get_opticalflow, fully fused path vs the op-by-op structure of the reference (both on the GPU)
from handobjectconsist_amd.warping import opticalflow
bad4 = 0
for case in range(min(n_cases, 200)):
    seed = seed0 + 300000 + case
    rng = np.random.default_rng(seed)
    B, is_ = int(rng.integers(1, 4)), int(rng.integers(24, 200))
    H, Wd = int(rng.integers(8, is_ + 1)), int(rng.integers(8, is_ + 1))
    s = synth.random_scene(B, seed=seed, image_size=is_)
    ren = Renderer(image_size=is_, R=torch.eye(3, device=dev)[None], t=torch.zeros(1, 3, device=dev), K=torch.ones(1, 3, 3, device=dev),
                   orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True)
    res = {}
    for fused in (True, False):
        opticalflow.USE_VERTEX_COLOR_RENDER = opticalflow.USE_FUSED_EPILOGUE = opticalflow.USE_FUSED_VERTEX_STAGE = fused
        v1 = t(s["verts1"]).requires_grad_(True)
        flows = opticalflow.get_opticalflow([v1, t(s["verts2"])], t(s["faces"]), [t(s["K1"]), t(s["K2"])], ren, orig_img_size=(Wd, H),
                                            detach_textures=False, detach_renders=True, ignore_face_idxs=synth.HAND_IGNORE_FACES)
        w = [torch.from_numpy(np.random.default_rng(seed).standard_normal(f.shape).astype(np.float32)).to(dev) for f in flows]
        (flows[0] * w[0]).sum().backward(retain_graph=True)
        res[fused] = ([f.detach().cpu().numpy() for f in flows], v1.grad.cpu().numpy())
    opticalflow.USE_VERTEX_COLOR_RENDER = opticalflow.USE_FUSED_EPILOGUE = opticalflow.USE_FUSED_VERTEX_STAGE = True
    msg = []
    for i in (0, 1):
        a, b_ = res[True][0][i], res[False][0][i]
        sup = int(((a != 0) != (b_ != 0)).sum())
        if sup > 6: msg.append(f"flow{i} support differs at {sup} px")
        same = (a != 0) == (b_ != 0)
        d = np.abs(np.where(same, a - b_, 0)).max(-1)
        # The two paths project the vertices with different kernels and agree to 1 ulp (6e-8 in NDC).  NMR's
        # barycentrics go through the inverse of the PIXEL-space vertex matrix, whose conditioning is
        # ~(coordinate / triangle size)^2 ~ 1e3-1e4 for these few-pixel faces: one ulp in a vertex moves the
        # interpolated flow by up to ~1e-3 relative on some pixels (debugged on seed 370155: the fused path
        # equals the numpy oracle bit for bit, the op-by-op path differs from both at 23 pixels by <= 6e-4).
        nbig = int((d > 1e-4 * max(float(np.abs(b_).max()), 1.0)).sum())  # flows are in pixels: relative to their scale
        if nbig > 0.05 * max(int((a[..., 0] != 0).sum()), 400) or d.max() > 0.1:  # gross errors only
            msg.append(f"flow{i}: {nbig} px differ by > 1e-4 relative (max {d.max():.2e}, scale {np.abs(b_).max():.1f})")
    ga, gb = res[True][1], res[False][1]
    e, sc = np.abs(ga - gb).max(), np.abs(gb).max() + 1e-12
    # (same conditioning; gross errors only -- and only where both paths rendered the same faces: the vertices of the two
    # paths differ by an ulp, which can hand a pixel to another of several sub-pixel faces (seed 600094: 0.1 px^2 faces
    # on a 44-pixel raster, one pixel's flow 0.85 apart) and with it the whole gradient of a vertex)
    same_winners = all(np.abs(res[True][0][i] - res[False][0][i]).max() <= 1e-2 for i in (0, 1))
    if same_winners and e > 0.15 * sc: msg.append(f"vertex grad err {e:.2e} (scale {sc:.2e})")
    # ... and the fused path (the one training runs: stacked 2B render) against the CPU oracle, tightly
    kw4 = dict(KW, orig_size=is_, image_size=is_, anti_aliasing=False, near=0.1, far=100, eps=1e-3)
    ref4 = W.get_opticalflow(R, [s["verts1"], s["verts2"]], s["faces"], [s["K1"], s["K2"]], kw4, orig_img_size=(Wd, H),
                             ignore_face_idxs=synth.HAND_IGNORE_FACES)
    for i in (0, 1):
        a, r_ = res[True][0][i], ref4[i]
        sup = int(((a != 0) != (r_ != 0)).sum())
        err = float(np.abs(a - r_).max()) if sup == 0 else float("inf")
        if sup or err > 1e-4 * max(float(np.abs(r_).max()), 1.0):
            msg.append(f"fused flow{i} vs ORACLE: support differs at {sup} px, max err {err:.2e}")
    if msg:
        bad4 += 1
        print(f"seed {seed} B={B} is={is_} crop {H}x{Wd}: " + "; ".join(msg))
print(f"sweep 4 (get_opticalflow fused vs op-by-op and vs the oracle): {min(n_cases, 200)} cases, {bad4} with mismatches")

# ---- fifth sweep: head post-processing kernels vs the op-by-op PyTorch code
model5 = synthnet.SynthMeshRegNet().to(dev).eval()
bad5 = 0
for case in range(min(n_cases, 300)):
    seed = seed0 + 400000 + case
    g = torch.Generator().manual_seed(seed)
    B, Vo = int(torch.randint(1, 40, (1,), generator=g)), int(torch.randint(1, 1500, (1,), generator=g))
    mk = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g)).to(dev)
    rs = float(10 ** torch.empty(1).uniform_(-5, 0.8, generator=g))
    pose, shape, st, so = mk(B, 18, s=0.3), mk(B, 10), mk(B, 3), mk(B, 6)
    so[:, 3:] *= rs
    K = torch.tensor([[350.0, 0.0, 120.0], [0.0, 350.0, 131.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).to(dev)
    K[:, 0, 0] += mk(B, s=40.0); K[:, 1, 1] = K[:, 0, 0]; K[:, :2, 2] += mk(B, 2, s=10.0)
    can = mk(B, Vo, 3, s=0.05)
    res_wh = (int(torch.randint(32, 640, (1,), generator=g)), int(torch.randint(32, 640, (1,), generator=g)))
    outs = {}
    for hip in (True, False):
        synthnet.USE_HIP_POST = hip
        leaves = [x.clone().requires_grad_(True) for x in (pose, shape, st, so)]
        o = model5.post_heads(*leaves, K, can, input_res=res_wh)
        ws = [torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(dev) for x in o]
        sum((a * w).sum() for a, w in zip(o, ws)).backward()
        outs[hip] = ([a.detach() for a in o], [l.grad for l in leaves])
    synthnet.USE_HIP_POST = True
    msg = []
    for a, b_, name in zip(outs[True][0], outs[False][0], ("handverts3d", "joints3d", "joints2d", "objverts3d", "objverts2d")):
        e, sc = float((a - b_).abs().max()), float(b_.abs().max()) + 1e-12
        if e > 2e-5 * sc: msg.append(f"{name} err {e:.2e} (scale {sc:.2e})")
    for a, b_, name in zip(outs[True][1], outs[False][1], ("pose", "shape", "scaletrans", "st_obj")):
        e, sc = float((a - b_).abs().max()), float(b_.abs().max()) + 1e-12
        if not torch.isfinite(a).all() or e > 5e-4 * sc: msg.append(f"grad {name} err {e:.2e} (scale {sc:.2e})")
    if msg:
        bad5 += 1
        print(f"seed {seed} B={B} Vo={Vo} rot scale {rs:.1e}: " + "; ".join(msg))
print(f"sweep 5 (head post-processing): {min(n_cases, 300)} cases, {bad5} with mismatches")

# ---- sixth sweep: trunk glue kernels (frozen BN + identity + ReLU; stem BN + ReLU + max-pool) vs the stock modules
import torch.nn.functional as TF
from handobjectconsist_amd.nn import frozen_bn
bad6 = 0
for case in range(min(n_cases, 300)):
    seed = seed0 + 500000 + case
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    N, C, H, Wd = ri(1, 9), ri(1, 70), ri(1, 70), ri(1, 70)
    if case % 7 == 0: H, Wd = 4 * ri(1, 20), 4 * ri(1, 20)
    stem = case % 3 == 0
    relu, with_res = bool(ri(0, 2)), bool(ri(0, 2)) and not stem
    bn = torch.nn.BatchNorm2d(C).to(dev).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) * 0.7 + 0.8); bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.4); bn.running_var.copy_(torch.rand(C, generator=g) * 2 + 0.02)
    x = torch.randn(N, C, H, Wd, generator=g).to(dev)
    res = torch.randn(N, C, H, Wd, generator=g).to(dev) if with_res else None
    dup = bool(ri(0, 2))  # the form the trainer launches: the activation as two autograd outputs, two gradients summed on load
    outs = {}
    for hip in (True, False):
        xs = x.clone().requires_grad_(True)
        rs_ = res.clone().requires_grad_(True) if with_res else None
        bn.zero_grad(set_to_none=True)
        if hip:
            y = frozen_bn.stem_pool(xs, bn, dup=dup) if stem else frozen_bn.bn_act(xs, bn, residual=rs_, relu=relu, dup=dup)
            y, y_dup = y if dup else (y, None)
        else:
            z = TF.batch_norm(xs, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
            zz = z if rs_ is None else z + rs_
            y = TF.max_pool2d(TF.relu(z), 3, 2, 1) if stem else (TF.relu(zz) if relu else zz)
        gg = torch.Generator().manual_seed(seed)
        gy, gy2 = torch.randn(y.shape, generator=gg).to(dev), torch.randn(y.shape, generator=gg).to(dev)
        if dup and hip: torch.autograd.backward([y, y_dup], [gy, gy2])
        else: y.backward(gy + gy2 if dup else gy)   # the reference on the sum of the two gradients
        outs[hip] = (y.detach(), xs.grad, bn.weight.grad.clone(), bn.bias.grad.clone(), None if rs_ is None else rs_.grad)
    msg = []
    a, b_ = outs[True], outs[False]
    sc = lambda t_: float(t_.abs().max()) + 1e-20
    if a[0].shape != b_[0].shape or float((a[0] - b_[0]).abs().max()) > 3e-6 * sc(b_[0]): msg.append("forward")
    nbad = int(((a[1] - b_[1]).abs() > 1e-5 * sc(b_[1])).sum())      # a ReLU mask / arg-max may flip where z rounds across a tie
    if nbad > max(3, x.numel() // 3000): msg.append(f"grad x differs at {nbad} of {x.numel()} elements")
    tol = 3e-5 if nbad == 0 else 2e-2
    for k, name in ((2, "grad weight"), (3, "grad bias")):
        if float((a[k] - b_[k]).abs().max()) > tol * sc(b_[k]): msg.append(f"{name} err {float((a[k] - b_[k]).abs().max()):.2e} (scale {sc(b_[k]):.2e})")
    if with_res and int(((a[4] - b_[4]).abs() > 1e-6 * sc(b_[4])).sum()) > max(3, x.numel() // 3000): msg.append("grad residual")
    if msg:
        bad6 += 1
        print(f"seed {seed} {'stem' if stem else 'bn_act'} shape {(N, C, H, Wd)} relu={relu} res={with_res} dup={dup}: " + "; ".join(msg))
print(f"sweep 6 (trunk glue kernels): {min(n_cases, 300)} cases, {bad6} with mismatches")

# ---- seventh sweep: frames -> batch (Pillow's nearest affine transform, bit-exact) vs the oracle
from handobjectconsist_amd.datasets import frames as frames_mod
from oracle import augment_ref as AR
bad7 = 0
for case in range(min(n_cases, 200)):
    seed = seed0 + 600000 + case
    rng = np.random.default_rng(seed)
    N, Hs, Ws = int(rng.integers(1, 5)), int(rng.integers(1, 90)), int(rng.integers(1, 90))
    Wo, Ho = int(rng.integers(1, 100)), int(rng.integers(1, 70))
    frames = rng.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8)
    coeffs = []
    for n in range(N):
        kind = int(rng.integers(0, 4))
        if kind == 0: a = [rng.uniform(0.1, 4) * rng.choice([-1, 1]), 0, rng.uniform(-30, 60), 0, rng.uniform(0.1, 4) * rng.choice([-1, 1]), rng.uniform(-30, 60)]
        elif kind == 1:
            th, s_ = rng.uniform(-3.2, 3.2), rng.uniform(0.2, 3)
            a = [s_ * np.cos(th), -s_ * np.sin(th), rng.uniform(-30, 60), s_ * np.sin(th), s_ * np.cos(th), rng.uniform(-30, 60)]
        elif kind == 2: a = [float(rng.integers(-2, 3)), float(rng.integers(-1, 2)), float(rng.integers(-5, 40)), float(rng.integers(-1, 2)), float(rng.integers(-2, 3)), float(rng.integers(-5, 40))]
        else: a = [rng.uniform(-2, 2) * 10.0 ** rng.integers(0, 5), rng.uniform(-1, 1), rng.uniform(-50000, 50000), rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(-40, 40)]
        coeffs.append([float(v) for v in a])
    flip = rng.random(N) < 0.3
    img, mask = frames_mod.frames_to_batch(t(frames), np.array(coeffs), (Wo, Ho), flip=flip)
    img, mask = img.cpu().numpy(), mask.cpu().numpy()
    ok = True
    for n in range(N):
        ref_u8, inside = AR.pil_affine_nearest(frames[n][:, ::-1] if flip[n] else frames[n], coeffs[n], (Wo, Ho))
        ref = (ref_u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)).transpose(2, 0, 1)
        ok = ok and np.array_equal(img[n], ref) and np.array_equal(mask[n, 0] == 1, inside)
    if not ok:
        bad7 += 1
        print(f"seed {seed} N={N} src {Hs}x{Ws} -> {Ho}x{Wo}: mismatch")
print(f"sweep 7 (frames -> batch): {min(n_cases, 200)} cases, {bad7} with mismatches")

# ---- eighth sweep: the pair as ONE fused node (opticalflow.flow_pair_loss: the path training takes since round 4) against
# ---- the CPU oracle (flows, both loss terms) and against the composed get_opticalflow + pair_consist path (vertex
# ---- gradient), whole meshes and (hand, object) parts, random raster sizes / crops / jitter borders / loss weights
bad8, skipped8 = 0, 0
for case in range(min(n_cases, 300)):
    seed = seed0 + 700000 + case
    rng = np.random.default_rng(seed)
    B, is_ = int(rng.integers(1, 5)), 4 * int(rng.integers(6, 56))  # (the node's backward reads pixel quads: rasters of 4 k pixels)
    H, Wd = (is_, is_) if rng.random() < 0.3 else (int(rng.integers(8, is_ + 1)), int(rng.integers(8, is_ + 1)))
    s = synth.random_scene(B, seed=seed, image_size=is_)
    if rng.random() < 0.2:  # a frame far off to the side / nothing rendered in one of the frames
        s["verts2"] = s["verts2"] + np.float32(rng.choice([0.3, 3.0]))
    ren = Renderer(image_size=is_, R=torch.eye(3, device=dev)[None], t=torch.zeros(1, 3, device=dev), K=torch.ones(1, 3, 3, device=dev),
                   orig_size=is_, anti_aliasing=False, fill_back=True, near=0.1, no_light=True)
    im_ref, im, jm_ref, jm = synth.random_images(B, H, Wd, seed)
    if rng.random() < 0.3: jm_ref, jm = jm_ref[:, :1], jm[:, :1]  # one-channel jitter masks
    gl = rng.standard_normal((2, B)).astype(np.float32)
    if rng.random() < 0.2: gl[1] = 0  # no gradient through the backward term
    msg = []
    v1 = t(s["verts1"]).requires_grad_(True)
    flows = opticalflow.get_opticalflow([v1, t(s["verts2"])], t(s["faces"]), [t(s["K1"]), t(s["K2"])], ren, orig_img_size=(Wd, H),
                                        ignore_face_idxs=synth.HAND_IGNORE_FACES)
    lc = imgflowarp.pair_consist(flows, t(im_ref), t(im), t(jm_ref), t(jm), PyramidCriterion("l1"), use_backward=True, outputs="loss")
    # (pair_consist's loss = forward + backward term; the node returns them separately: compare through two weightings)
    parts = bool(rng.random() < 0.5)
    if parts:
        nh = 778
        h1, o1 = t(s["verts1"][:, :nh]).requires_grad_(True), t(s["verts1"][:, nh:]).requires_grad_(True)
        vf = [(h1, o1), (t(s["verts2"][:, :nh]), t(s["verts2"][:, nh:]))]
        fh = s["faces"][0, :1552]
        assert (s["faces"][:, :1552] == fh).all() and s["faces"][:, 1552:].min() >= nh
        ff = (t(fh), t(s["faces"][:, 1552:] - nh))
    else:
        v1f = t(s["verts1"]).requires_grad_(True)
        vf, ff = [v1f, t(s["verts2"])], t(s["faces"])
    fused = opticalflow.flow_pair_loss(vf, ff, [t(s["K1"]), t(s["K2"])], ren, (Wd, H), t(im_ref), t(im), t(jm_ref), t(jm),
                                       ignore_face_idxs=synth.HAND_IGNORE_FACES)
    if fused is None:
        skipped8 += 1
        continue
    kw8 = dict(KW, orig_size=is_, image_size=is_, anti_aliasing=False, near=0.1, far=100, eps=1e-3)
    ref_flows = W.get_opticalflow(R, [s["verts1"], s["verts2"]], s["faces"], [s["K1"], s["K2"]], kw8, orig_img_size=(Wd, H),
                                  ignore_face_idxs=synth.HAND_IGNORE_FACES)
    ref_fwd = W.pair_consist(ref_flows, im_ref, im, jm_ref, jm, False)[0]
    ref_both = W.pair_consist(ref_flows, im_ref, im, jm_ref, jm, True)[0]
    lf, lb = fused[0].detach().cpu().numpy(), fused[1].detach().cpu().numpy()
    for got, want, name in ((lf, ref_fwd, "loss_fwd"), (lf + lb, ref_both, "loss_fwd + loss_bwd")):
        e = np.abs(got - want).max()
        if e > 2e-5 * max(1.0, np.abs(want).max()): msg.append(f"{name} vs ORACLE err {e:.2e}")
    # the node's flows: defined under covered tiles, equal to the oracle's there; the oracle's flow is zero elsewhere
    tiles = getattr(fused[2][0], "_hoc_coverage", None)
    for i in (0, 1):
        a, r_ = fused[2][i].detach().cpu().numpy(), ref_flows[i]
        cov = r_[..., 0] != 0
        e = float(np.abs(a - r_)[cov].max()) if cov.any() else 0.0
        if e > 1e-4 * max(float(np.abs(r_).max()), 1.0): msg.append(f"flow{i} under the render vs ORACLE err {e:.2e}")
    # gradient: (gl[0] . loss_fwd + gl[1] . loss_bwd) -- the composed path needs the two terms apart
    l_fwd_c = imgflowarp.pair_consist(flows, t(im_ref), t(im), t(jm_ref), t(jm), PyramidCriterion("l1"), use_backward=False, outputs="loss")[0]
    l_bwd_c = lc[0] - l_fwd_c
    ((l_fwd_c * t(gl[0])).sum() + (l_bwd_c * t(gl[1])).sum()).backward()
    ((fused[0] * t(gl[0])).sum() + (fused[1] * t(gl[1])).sum()).backward()
    gc = v1.grad
    gf = torch.cat([h1.grad, o1.grad], 1) if parts else v1f.grad
    if not torch.isfinite(gf).all(): msg.append("vertex gradient non-finite")
    e, sc = float((gf - gc).abs().max()), float(gc.abs().max())
    if e > 2e-4 * sc + 1e-12: msg.append(f"vertex gradient vs composed path err {e:.2e} (scale {sc:.2e})")
    if msg:
        bad8 += 1
        print(f"seed {seed} B={B} is={is_} crop {H}x{Wd} parts={parts}: " + "; ".join(msg))
print(f"sweep 8 (fused pair node vs oracle / composed path): {min(n_cases, 300)} cases, {skipped8} not applicable, {bad8} with mismatches")
sys.exit(1 if (bad or bad2 or bad3 or bad4 or bad5 or bad6 or bad7 or bad8) else 0)
