"""CPU oracle for the warp half of the hot path (numpy, vectorised).

TEST INFRASTRUCTURE ONLY: imported by tests/, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of bench.py.  The shipped package never imports it.

PINNED: unlike the render half, the functions restated here exist in /root/reference
(meshreg/warping/imgflowarp.py, meshreg/optim/lossutils.py, pyramidloss.py:56-62) and
import on CPU; tests/golden/warp_*.npz were generated from the real reference by
tests/golden/make_golden_warp.py and this file is checked against them in
tests/test_oracle_warp.py.  The only third-party arithmetic is torch's
``grid_sample`` (zeros padding, align_corners=False), restated from the published
formula ``ix = ((x + 1) * W - 1) / 2`` (bilinear: 4 taps, weights from the opposite
corner; nearest: round-half-even).
"""
import numpy as np

F32 = np.float32


def get_spatial_meshgrid(shape, scale=False):
    """imgflowarp.get_spatial_meshgrid (imgflowarp.py:8-28) for x of shape [B,C,H,W]."""
    B, _, H, W = shape
    xx = np.broadcast_to(np.arange(W, dtype=F32)[None, :], (H, W))
    yy = np.broadcast_to(np.arange(H, dtype=F32)[:, None], (H, W))
    grid = np.stack([xx, yy], 0)[None].repeat(B, 0).astype(F32)
    if scale:
        grid[:, 0] = grid[:, 0] / F32(W)
        grid[:, 1] = grid[:, 1] / F32(H)
    return grid


def _unnormalize(coord, size):
    # align_corners=False: ((coord + 1) * size - 1) / 2, fp32 op by op
    return ((coord + F32(1)) * F32(size) - F32(1)) / F32(2)


def _gather(x, iy, ix):
    """x[B,C,H,W] sampled at integer (iy, ix)[B,H,W] with zeros padding -> [B,C,H,W], inb[B,H,W]."""
    B, C, H, W = x.shape
    inb = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    ixc = np.clip(ix, 0, W - 1).astype(np.int64)
    iyc = np.clip(iy, 0, H - 1).astype(np.int64)
    b = np.arange(B)[:, None, None]
    vals = x[b, :, iyc, ixc]  # [B,H,W,C]
    vals = np.moveaxis(vals, -1, 1)
    # a tap outside the image is SKIPPED (grid_sample's within_bounds test), not multiplied by zero: what the clamped address
    # holds -- a NaN, say -- never reaches the result
    return np.where(inb[:, None], vals, F32(0)).astype(F32), inb


def grid_sample(x, vgrid, mode="bilinear", with_grad=False):
    """torch.nn.functional.grid_sample(x, vgrid[B,H,W,2], mode, 'zeros', align_corners=False).

    with_grad=True additionally returns (d out / d ix, d out / d iy) per channel, in
    UNNORMALISED pixel units (bilinear only)."""
    x = np.ascontiguousarray(x, F32)
    B, C, H, W = x.shape
    ix = _unnormalize(vgrid[..., 0].astype(F32), W)
    iy = _unnormalize(vgrid[..., 1].astype(F32), H)
    if mode == "nearest":
        ixn = np.rint(ix)
        iyn = np.rint(iy)
        ok = np.isfinite(ixn) & np.isfinite(iyn)
        ixn = np.where(ok, ixn, -10).astype(np.int64)
        iyn = np.where(ok, iyn, -10).astype(np.int64)
        out, _ = _gather(x, iyn, ixn)
        return out.astype(F32)
    ix_nw = np.floor(ix)
    iy_nw = np.floor(iy)
    ix_ne, iy_ne = ix_nw + 1, iy_nw
    ix_sw, iy_sw = ix_nw, iy_nw + 1
    ix_se, iy_se = ix_nw + 1, iy_nw + 1
    with np.errstate(invalid="ignore"):  # (inf - inf at a non-finite position: NaN weights, and no tap in bounds)
        nw = (ix_se - ix) * (iy_se - iy)
        ne = (ix - ix_sw) * (iy_sw - iy)
        sw = (ix_ne - ix) * (iy - iy_ne)
        se = (ix - ix_nw) * (iy - iy_nw)

    def toint(a):
        a = np.where(np.isfinite(a), a, -10)
        return np.clip(a, -10, 1 << 30).astype(np.int64)

    v_nw, b_nw = _gather(x, toint(iy_nw), toint(ix_nw))
    v_ne, b_ne = _gather(x, toint(iy_ne), toint(ix_ne))
    v_sw, b_sw = _gather(x, toint(iy_sw), toint(ix_sw))
    v_se, b_se = _gather(x, toint(iy_se), toint(ix_se))

    def tap(inb, v, w):
        # a skipped tap adds nothing, whatever its weight is (a non-finite position has non-finite weights and no tap in bounds:
        # the sample is 0, as where the float-to-int conversion of such a position saturates)
        with np.errstate(invalid="ignore"):
            return np.where(inb[:, None], v * w[:, None], F32(0)).astype(F32)

    out = tap(b_nw, v_nw, nw) + tap(b_ne, v_ne, ne) + tap(b_sw, v_sw, sw) + tap(b_se, v_se, se)
    out = out.astype(F32)
    if not with_grad:
        return out
    with np.errstate(invalid="ignore"):
        gix = (-tap(b_nw, v_nw, iy_se - iy) + tap(b_ne, v_ne, iy_sw - iy)
               - tap(b_sw, v_sw, iy - iy_ne) + tap(b_se, v_se, iy - iy_nw))
        giy = (-tap(b_nw, v_nw, ix_se - ix) - tap(b_ne, v_ne, ix - ix_sw)
               + tap(b_sw, v_sw, ix_ne - ix) + tap(b_se, v_se, ix - ix_nw))
    return out, gix.astype(F32), giy.astype(F32)


def _vgrid(flow):
    """imgflowarp.py:41-48: grid + flow, normalised by (W-1), (H-1)."""
    B, _, H, W = flow.shape
    grid = get_spatial_meshgrid((B, 2, H, W))
    v = grid + flow.astype(F32)
    vx = F32(2.0) * v[:, 0] / F32(max(W - 1, 1)) - F32(1.0)
    vy = F32(2.0) * v[:, 1] / F32(max(H - 1, 1)) - F32(1.0)
    return np.stack([vx, vy], -1).astype(F32)


def warp(x, flow, thresh=0.99999, mode="bilinear"):
    """imgflowarp.warp (imgflowarp.py:31-55) -> (output * mask, mask)."""
    x = np.ascontiguousarray(x, F32)
    vgrid = _vgrid(flow)
    output = grid_sample(x, vgrid, mode)
    mask = grid_sample(np.ones_like(x), vgrid, mode)
    mask = np.where(mask < F32(thresh), F32(0), mask)
    mask = np.where(mask > 0, F32(1), mask).astype(F32)
    return (output * mask).astype(F32), mask


def warp_backward(x, flow, grad_out, thresh=0.99999):
    """Adjoint of warp (bilinear) w.r.t. flow -> [B,2,H,W] (the mask carries no gradient,
    SURVEY Q7) and w.r.t. x -> [B,C,H,W]."""
    x = np.ascontiguousarray(x, F32)
    B, C, H, W = x.shape
    vgrid = _vgrid(flow)
    _, gix, giy = grid_sample(x, vgrid, "bilinear", with_grad=True)
    _, mask = warp(x, flow, thresh)
    g = grad_out.astype(F32) * mask
    # chain: ix = ((vx+1)*W-1)/2, vx = 2 (x+u)/(W-1) - 1  =>  d ix / d u = W / (W-1)
    sx = F32(W) / F32(2) * (F32(2.0) / F32(max(W - 1, 1)))
    sy = F32(H) / F32(2) * (F32(2.0) / F32(max(H - 1, 1)))
    gflow = np.stack([(g * gix).sum(1) * sx, (g * giy).sum(1) * sy], 1).astype(F32)
    # grad wrt x: scatter of the four taps
    ix = _unnormalize(vgrid[..., 0], W)
    iy = _unnormalize(vgrid[..., 1], H)
    x0 = np.floor(ix)
    y0 = np.floor(iy)
    gx = np.zeros((B, C, H, W), np.float64)
    with np.errstate(invalid="ignore"):  # (a non-finite position: NaN weights of taps that are not in bounds)
        taps = [(0, 0, (x0 + 1 - ix) * (y0 + 1 - iy)), (1, 0, (ix - x0) * (y0 + 1 - iy)),
                (0, 1, (x0 + 1 - ix) * (iy - y0)), (1, 1, (ix - x0) * (iy - y0))]
    bidx = np.arange(B)[:, None, None].repeat(H, 1).repeat(W, 2)
    for dx, dy, w in taps:
        xi = (x0 + dx)
        yi = (y0 + dy)
        ok = np.isfinite(xi) & np.isfinite(yi) & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        xi_ = np.where(ok, xi, 0).astype(np.int64)
        yi_ = np.where(ok, yi, 0).astype(np.int64)
        for c in range(C):
            np.add.at(gx[:, c], (bidx[ok], yi_[ok], xi_[ok]), (g[:, c] * w)[ok])
    return gflow, gx.astype(F32)


def batch_masked_mean_loss(dists, mask):
    """lossutils.batch_masked_mean_loss (lossutils.py:1-8)."""
    mask = mask.astype(F32)
    axes = tuple(range(1, dists.ndim))
    batch_sum = (mask * dists).sum(axis=axes, dtype=np.float64)
    valid = mask.sum(axis=axes, dtype=np.float64)
    valid[valid == 0] = 1
    return (batch_sum / valid).astype(F32)


def pair_consist(recons_flow, image_ref, image, jitter_mask_ref, jitter_mask, use_backward=False,
                 thresh=0.99999, criterion="l1"):
    """imgflowarp.pair_consist (imgflowarp.py:58-115) with PyramidCriterion('l1') -- or 'l2': the squared
    difference, torch.nn.MSELoss(reduction="none") --, level_nb=1 (pyramidloss.py:56-62).
    recons_flow = [flow12, flow21], each [B,H,W,2]."""
    assert criterion in ("l1", "l2")
    f0 = recons_flow[0].transpose(0, 3, 1, 2)
    f1 = recons_flow[1].transpose(0, 3, 1, 2)
    warp1, warp_mask1 = warp(image_ref, f1, thresh)
    warpjitter1, _ = warp(jitter_mask_ref, f0, thresh)
    warp2, warp_mask2 = warp(image, f0, thresh)
    warpjitter2, _ = warp(jitter_mask, f1, thresh)
    warp_mask1 = warp_mask1 * (warpjitter2 == 1).astype(F32)
    warp_mask2 = warp_mask2 * (warpjitter1 == 1).astype(F32)
    flow_mask1 = ~(recons_flow[1] == 0)
    valid_mask1 = (warp_mask1[:, 0] != 0) & flow_mask1[..., 0] & (jitter_mask[:, 0] == 1)
    flow_mask2 = ~(recons_flow[0] == 0)
    valid_mask2 = (warp_mask2[:, 0] != 0) & flow_mask2[..., 0] & (jitter_mask_ref[:, 0] == 1)
    diff_fwd = warp1 - image.astype(F32)
    diff_bwd = warp2 - image_ref.astype(F32)
    diff_fwd, diff_bwd = (np.abs(diff_fwd), np.abs(diff_bwd)) if criterion == "l1" else (diff_fwd * diff_fwd, diff_bwd * diff_bwd)
    m1 = np.repeat(valid_mask1[:, None], 3, 1)
    m2 = np.repeat(valid_mask2[:, None], 3, 1)
    losses_fwd = batch_masked_mean_loss(diff_fwd, m1)
    losses_bwd = batch_masked_mean_loss(diff_bwd, m2)
    warp_loss = losses_bwd + losses_fwd if use_backward else losses_fwd
    masks = [
        {"warp_mask": warp_mask1, "full_mask": valid_mask1, "flow_mask": flow_mask1},
        {"warp_mask": warp_mask2, "full_mask": valid_mask2, "flow_mask": flow_mask2},
    ]
    return warp_loss.astype(F32), masks, [warp1, warp2], [diff_fwd, diff_bwd], (losses_fwd, losses_bwd)


def pair_consist_grad(recons_flow, image_ref, image, jitter_mask_ref, jitter_mask, grad_loss,
                      use_backward=False, thresh=0.99999, criterion="l1"):
    """d (sum_b grad_loss[b] * warp_loss[b]) / d recons_flow -> [g_flow12, g_flow21], [B,H,W,2]."""
    _, masks, warps, _, _ = pair_consist(recons_flow, image_ref, image, jitter_mask_ref, jitter_mask,
                                         use_backward, thresh, criterion)
    f0 = recons_flow[0].transpose(0, 3, 1, 2)
    f1 = recons_flow[1].transpose(0, 3, 1, 2)
    B = image.shape[0]
    out = []
    for flow, src, tgt, warped, m in (
        (f1, image_ref, image, warps[0], masks[0]["full_mask"]),
        (f0, image, image_ref, warps[1], masks[1]["full_mask"]),
    ):
        cnt = np.maximum(3.0 * m.reshape(B, -1).sum(1), 1.0)
        cnt[m.reshape(B, -1).sum(1) == 0] = 1
        res = warped - tgt.astype(F32)
        g = (np.sign(res) if criterion == "l1" else F32(2) * res) * m[:, None].astype(F32)
        g = g * (grad_loss.astype(F32) / cnt.astype(F32))[:, None, None, None]
        gflow, _ = warp_backward(src, flow, g.astype(F32), thresh)
        out.append(gflow.transpose(0, 2, 3, 1).astype(F32))
    g21, g12 = out
    if not use_backward:
        g12 = np.zeros_like(g12)
    return [g12, g21]


def occlusion_mask_from_warped_grid(grid, warped_grid, distance_thresh=0.03):
    """imgflowarp.occlusion_mask_from_warped_grid (imgflowarp.py:149-172); [B,H,W,4] inputs."""
    mask = grid[..., 2] * warped_grid[..., 2]
    d = ((warped_grid - grid) * mask[..., None])[..., :2].astype(F32)
    displ = np.sqrt((d * d).sum(-1, dtype=F32))
    motion = (displ < F32(distance_thresh)).astype(F32)
    return (mask * motion).astype(F32)


def get_occlusion_mask(mask_flow1, mask_flow2, flow12, flow21, thresh=0.99999):
    """imgflowarp.get_occlusion_mask (imgflowarp.py:118-146).  mask_flow*[B,1,H,W],
    flow*[B,3,H,W] -> occl_mask1, occl_mask2 [B,H,W]."""
    shp = mask_flow1.shape
    grid1 = np.concatenate([get_spatial_meshgrid(shp, True), mask_flow1, mask_flow1], 1).astype(F32)
    grid2 = np.concatenate([get_spatial_meshgrid(shp, True), mask_flow2, mask_flow2], 1).astype(F32)
    warp_grid12, _ = warp(grid1, flow21[:, :2], thresh, "nearest")
    warp_grid21, _ = warp(grid2, flow12[:, :2], thresh, "nearest")
    warp_grid12 = warp_grid12 * mask_flow2[:, :1]
    warp_grid21 = warp_grid21 * mask_flow1[:, :1]
    warp_grid212, _ = warp(warp_grid12, flow12[:, :2], thresh, "nearest")
    warp_grid121, _ = warp(warp_grid21, flow21[:, :2], thresh, "nearest")
    warp_grid212 = warp_grid212 * mask_flow1[:, :1]
    warp_grid121 = warp_grid121 * mask_flow2[:, :1]
    occl1 = occlusion_mask_from_warped_grid(grid1.transpose(0, 2, 3, 1), warp_grid212.transpose(0, 2, 3, 1))
    occl2 = occlusion_mask_from_warped_grid(grid2.transpose(0, 2, 3, 1), warp_grid121.transpose(0, 2, 3, 1))
    return occl1, occl2


def get_opticalflow(raster, verts_cam, faces_idx, camintrs, renderer_kw, orig_img_size=None,
                    mask_occlusions=True, ignore_face_idxs=None, return_renders=False, return_masks=False):
    """opticalflow.get_opticalflow (opticalflow.py:51-156) on top of the render oracle.
    `raster` is the oracle.raster_ref module; renderer_kw are the Renderer settings of
    warpreg.py:40-51 (image_size, R, t, dist_coeffs, orig_size, near, far, eps...).
    return_masks (with return_renders): a third element, the factor [B,1,is,is] each direction's render
    is multiplied with before the crop (the product of every mask on its way, image orientation)."""
    loc1 = raster.batch_proj2d(verts_cam[0], camintrs[0])
    loc2 = raster.batch_proj2d(verts_cam[1], camintrs[1])
    outs = []
    for (v, K, displ) in ((verts_cam[0], camintrs[0], loc2 - loc1), (verts_cam[1], camintrs[1], loc1 - loc2)):
        sample_flows = np.concatenate([displ, np.ones_like(displ[:, :, :1])], -1)
        tex = raster.batch_vertex_textures(faces_idx, sample_flows)
        ro = raster.render(v, faces_idx, tex, K, **renderer_kw)
        mask = (ro["alpha"][:, None] > F32(0.99999)).astype(F32)
        if ignore_face_idxs is not None:
            fim = ro["face_index_map"]
            ign = np.abs(fim[..., None] - np.asarray(ignore_face_idxs, np.int32)).min(-1) != 0
            ign = ign[:, ::-1]
            mask = mask * ign.astype(F32)[:, None]
        outs.append((ro, mask, ro["rgb"] * mask))
    (ro1, mask_flow1, pred12), (ro2, mask_flow2, pred21) = outs
    factors = [mask_flow1, mask_flow2]
    if mask_occlusions:
        mask_flow2 = ro2["alpha"][:, None].astype(F32)  # raw alpha
        occl1, occl2 = get_occlusion_mask(mask_flow1, mask_flow2, pred12, pred21)
        mask_flow1 = mask_flow1 * occl1[:, None]
        mask_flow2 = mask_flow2 * occl2[:, None]
        pred12 = pred12 * mask_flow1
        pred21 = pred21 * mask_flow2
        factors = [factors[0] * mask_flow1, factors[1] * mask_flow2]
    pred12 = pred12.transpose(0, 2, 3, 1)[..., :2]
    pred21 = pred21.transpose(0, 2, 3, 1)[..., :2]
    if orig_img_size is not None:
        pred12 = pred12[:, : orig_img_size[1], : orig_img_size[0]]
        pred21 = pred21[:, : orig_img_size[1], : orig_img_size[0]]
    flows = [np.ascontiguousarray(pred12, F32), np.ascontiguousarray(pred21, F32)]
    if return_renders:
        return (flows, [ro1, ro2], factors) if return_masks else (flows, [ro1, ro2])
    return flows


# texel (i, j, k) of a 2 x 2 x 2 texture has flat index 4 i + 2 j + k: batch_vertex_textures puts the colour of a face's
# vertex 0 / 1 / 2 at (1,0,0) / (0,1,0) / (0,0,1), and fill_back's transposed texture keeps that true of the reversed face
_VERTEX_TEXELS = ((0, 4), (1, 2), (2, 1))


def _vertex_colour_grad(raster, ro, faces2, grad_rgb_map, num_verts, fp32):
    """Adjoint of texture sampling + fill_back + batch_vertex_textures for vertex-colour textures: the sampling weights of
    each covered pixel that fall on one of its face's three vertex texels, times the pixel's gradient, added to that vertex.
    grad_rgb_map [B,is,is,3] in RASTER orientation -> [B,V,3].  float64 sums (np.add.at), or with ``fp32`` the chain's
    existing fp32 pieces: raster.backward_textures (kernel E, serial fp32 sums) and an fp32 scatter of its texels."""
    sv = ro["_saved"]
    fim, swgt, sidx = sv["face_index_map"], sv["sampling_weight_map"], sv["sampling_index_map"]
    B = fim.shape[0]
    if fp32:
        gt = raster.backward_textures(fim, swgt, sidx, grad_rgb_map.astype(F32), faces2.shape[1], 2).reshape(B, faces2.shape[1], 8, 3)
        gcol = np.zeros((B, num_verts, 3), F32)
        for b in range(B):
            for slot, texel in _VERTEX_TEXELS:
                np.add.at(gcol[b], faces2[b, :, slot], gt[b, :, texel])
        return gcol
    b, y, x = np.nonzero(fim >= 0)
    f = fim[b, y, x]
    g = grad_rgb_map[b, y, x].astype(np.float64)
    gcol = np.zeros((B, num_verts, 3), np.float64)
    for pn in range(8):
        isc, w = sidx[b, y, x, pn], swgt[b, y, x, pn].astype(np.float64)
        for slot, texel in _VERTEX_TEXELS:
            sel = isc == texel
            np.add.at(gcol, (b[sel], faces2[b[sel], f[sel], slot]), w[sel, None] * g[sel])
    return gcol


def _proj2d_grad(verts, camintr, grad_loc, dtype):
    """Adjoint of raster.batch_proj2d: loc = (K v)[:2] / (K v)[2]; grad_loc [B,V,2] -> [B,V,3]."""
    v, K, g = verts.astype(dtype), camintr.astype(dtype), grad_loc.astype(dtype)
    h = np.matmul(v, K.transpose(0, 2, 1))
    gh = np.stack([g[..., 0] / h[..., 2], g[..., 1] / h[..., 2],
                   -(g[..., 0] * h[..., 0] + g[..., 1] * h[..., 1]) / (h[..., 2] * h[..., 2])], -1)
    return np.matmul(gh, K)


def get_opticalflow_vertex_grad(raster, verts_cam, faces_idx, camintrs, renderer_kw, grad_flows, orig_img_size=None,
                                ignore_face_idxs=None, forward=None, fp32=False):
    """d (sum flow12 * grad_flows[0] + sum flow21 * grad_flows[1]) / d (verts1, verts2) of ``get_opticalflow`` in the
    reference's training graph (opticalflow.py:51-156 with detach_textures=False, detach_renders=True): the renders are
    detached, so geometry gets no gradient through the rasteriser, and every mask is a constant -- the vertices enter through
    the two displacement textures alone.  Built from the oracle's FORWARD decision maps (face index, sampling weights, masks,
    occlusion), then, in float64: the adjoint of the crop and the mask products, the scatter of each covered pixel's sampling
    weights to its face's vertices (what kernel E and the adjoints of fill_back and batch_vertex_textures amount to for
    vertex-colour textures) and the adjoint of batch_proj2d.  Returns (grad_verts1, grad_verts2), float64 [B,V,3].

    ``forward``: the ``(renders, factors)`` of a ``get_opticalflow(..., return_renders=True, return_masks=True)`` call on the
    same arguments with ``keep_saved=True`` among the renderer settings (spares the two renders).  ``fp32``: the same chain
    with its existing fp32 pieces (raster.backward_textures, fp32 sums and products) -- what an fp32 implementation in the
    reference's order of operations gives; float32 result."""
    dtype = F32 if fp32 else np.float64
    if forward is None:
        _, renders, factors = get_opticalflow(raster, verts_cam, faces_idx, camintrs, dict(renderer_kw, keep_saved=True), orig_img_size,
                                              True, ignore_face_idxs, return_renders=True, return_masks=True)
    else:
        renders, factors = forward
    B, V = verts_cam[0].shape[:2]
    is_ = renders[0]["_saved"]["face_index_map"].shape[1]
    faces_idx = np.asarray(faces_idx)
    faces2 = raster.fill_back(faces_idx)[0] if renderer_kw.get("fill_back_", True) else faces_idx
    gcols = []
    for ro, factor, g in zip(renders, factors, grad_flows):
        H, W = g.shape[1:3]
        full = np.zeros((B, is_, is_, 3), dtype)
        full[:, :H, :W, :2] = g  # (adjoint of the crop and of dropping the third channel)
        full = full * factor[:, 0, :, :, None].astype(dtype)  # (... of the mask products)
        gcols.append(_vertex_colour_grad(raster, ro, faces2, full[:, ::-1], V, fp32))  # (... of the vertical flip)
    # colours of render 1: (loc2 - loc1, 1); of render 2: (loc1 - loc2, 1)
    g_loc2 = gcols[0][..., :2] - gcols[1][..., :2]
    return (_proj2d_grad(verts_cam[0], camintrs[0], -g_loc2, dtype), _proj2d_grad(verts_cam[1], camintrs[1], g_loc2, dtype))
