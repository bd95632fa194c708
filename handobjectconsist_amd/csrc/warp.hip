// warp.hip -- photometric warp kernels for gfx950 (MI355X), the dense launches (one workgroup per block of every image).
// The listed launches of the training path (mr_*_tiles) are in warp_tiles.hip; the device functions both use are in
// warp_device.hpp.
//
// Replaces the PyTorch op chains of /root/reference/meshreg/warping/imgflowarp.py:
//   warp (:31-55)                  -> warp_forward_kernel / warp_backward_kernel
//   get_occlusion_mask (:118-172)  -> occlusion_kernel (four chained nearest warps fused into
//                                     two dependent gathers per pixel, no intermediates)
//   pair_consist (:58-115) + PyramidCriterion('l1').compute (pyramidloss.py:56-62) +
//   batch_masked_mean_loss (lossutils.py:1-8)
//                                  -> pair_consist_forward_kernel (both directions, 8 grid
//                                     samples, mask algebra and the masked L1 sums in ONE pass
//                                     over the pixels) + finalize + backward w.r.t. the flows.
//   opticalflow.py:109-154 mask algebra / crop / permute
//                                  -> flow_mask_kernel, flow_finalize_{forward,backward}_kernel
// All are HBM-streaming kernels: one lane per pixel, channel planes read coalesced, the
// bilinear taps hit L1/L2 (flows are a few pixels); in the pair kernels the two taps of a row
// come from ONE 8-byte load at a 32-bit offset from a wave-uniform plane pointer (load-instruction
// count is what bounds them).  Reductions are two-stage and deterministic (fixed-order block
// partials -> per-sample finalize), no float atomics.
//
// grid_sample semantics restated (torch, zeros padding, align_corners=False):
//   vx = 2 (x + u) / max(W - 1, 1) - 1 ;  ix = ((vx + 1) W - 1) / 2        
//
// Kernels, in file order: warp_forward_kernel, warp_backward_kernel, occlusion_kernel, occlusion_flow_kernel,
// flow_mask_kernel, flow_finalize_forward_kernel, flow_finalize_backward_kernel, pair_consist_finalize_kernel,
// pair_consist_forward_kernel, pair_consist_forward_l2_kernel, pair_consist_backward_kernel, pair_consist_backward_l2_kernel.
//
// Entry points: mr_warp_forward, mr_warp_backward, mr_occlusion_mask, mr_occlusion_flow, mr_pair_consist_workspace_bytes,
// mr_pair_consist_forward[_crit], mr_pair_consist_backward[_crit], mr_flow_mask, mr_flow_finalize_forward,
// mr_flow_finalize_backward.
#include <algorithm>

#include "mr_common.hpp"
#include "pair_launch.hpp"
#include "warp_device.hpp"

namespace mr {

// ---------------------------------------------------------------------------------------
// warp
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) warp_forward_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ flow,
                                                           float* __restrict__ out, float* __restrict__ mask,
                                                           int B, int C, int H, int W, float thresh, int mode) {
    const int64_t hw = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * hw) return;
    const int b = (int)(i / hw);
    const int64_t pix = i % hw;
    const int yy = (int)(pix / W), xx = (int)(pix % W);
    const float u = flow[((int64_t)b * 2 + 0) * hw + pix], v = flow[((int64_t)b * 2 + 1) * hw + pix];
    float ix, iy;
    sample_pos((float)xx, (float)yy, u, v, W, H, ix, iy);
    if (mode == 0) {
        const Taps t = make_taps(ix, iy);
        const float m = valid_mask(t, W, H, thresh);
        for (int c = 0; c < C; c++) {
            const int64_t o = ((int64_t)b * C + c) * hw;
            out[o + pix] = bilin(x + o, t, W, H) * m;
            mask[o + pix] = m;
        }
    } else {
        int xn, yn;
        nearest_idx(ix, iy, xn, yn);
        const bool ok = inb(xn, yn, W, H);
        float m = ok ? 1.0f : 0.0f;
        if (m < thresh) m = 0.0f;
        if (m > 0.0f) m = 1.0f;
        for (int c = 0; c < C; c++) {
            const int64_t o = ((int64_t)b * C + c) * hw;
            const float s = ok ? x[o + (int64_t)yn * W + xn] : 0.0f;
            out[o + pix] = s * m;
            mask[o + pix] = m;
        }
    }
}

__global__ void __launch_bounds__(256) warp_backward_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ flow,
                                                            const float* __restrict__ grad_out,
                                                            float* __restrict__ grad_x,
                                                            float* __restrict__ grad_flow, int B, int C, int H,
                                                            int W, float thresh, int mode) {
    const int64_t hw = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * hw) return;
    const int b = (int)(i / hw);
    const int64_t pix = i % hw;
    const int yy = (int)(pix / W), xx = (int)(pix % W);
    const float u = flow[((int64_t)b * 2 + 0) * hw + pix], v = flow[((int64_t)b * 2 + 1) * hw + pix];
    float ix, iy;
    sample_pos((float)xx, (float)yy, u, v, W, H, ix, iy);
    float gu = 0.0f, gv = 0.0f;
    if (mode == 0) {
        const Taps t = make_taps(ix, iy);
        const float m = valid_mask(t, W, H, thresh);
        for (int c = 0; c < C; c++) {
            const int64_t o = ((int64_t)b * C + c) * hw;
            const float g = grad_out[o + pix] * m;
            if (grad_flow) {
                float gix, giy;
                bilin_grad(x + o, t, W, H, gix, giy);
                gu += g * gix;
                gv += g * giy;
            }
            if (grad_x && g != 0.0f) {
                if (inb(t.x0, t.y0, W, H)) atomicAdd(&grad_x[o + (int64_t)t.y0 * W + t.x0], g * t.nw);
                if (inb(t.x0 + 1, t.y0, W, H)) atomicAdd(&grad_x[o + (int64_t)t.y0 * W + t.x0 + 1], g * t.ne);
                if (inb(t.x0, t.y0 + 1, W, H)) atomicAdd(&grad_x[o + (int64_t)(t.y0 + 1) * W + t.x0], g * t.sw);
                if (inb(t.x0 + 1, t.y0 + 1, W, H))
                    atomicAdd(&grad_x[o + (int64_t)(t.y0 + 1) * W + t.x0 + 1], g * t.se);
            }
        }
        // d ix / d u = (W / 2) * (2 / max(W - 1, 1))
        gu = gu * ((float)W / 2.0f) * (2.0f / (float)max(W - 1, 1));
        gv = gv * ((float)H / 2.0f) * (2.0f / (float)max(H - 1, 1));
    } else if (grad_x) {
        int xn, yn;
        nearest_idx(ix, iy, xn, yn);
        if (inb(xn, yn, W, H)) {
            float m = 1.0f;
            if (m < thresh) m = 0.0f;
            for (int c = 0; c < C; c++) {
                const int64_t o = ((int64_t)b * C + c) * hw;
                const float g = grad_out[o + pix] * m;
                if (g != 0.0f) atomicAdd(&grad_x[o + (int64_t)yn * W + xn], g);
            }
        }
    }
    if (grad_flow) {
        grad_flow[((int64_t)b * 2 + 0) * hw + pix] = gu;
        grad_flow[((int64_t)b * 2 + 1) * hw + pix] = gv;
    }
}

// ---------------------------------------------------------------------------------------
// forward-backward occlusion check
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) occlusion_kernel(const float* __restrict__ mask1,
                                                        const float* __restrict__ mask2,
                                                        const float* __restrict__ flow12,
                                                        const float* __restrict__ flow21, int64_t fbstride,
                                                        const float* __restrict__ scale12,
                                                        const float* __restrict__ scale21,
                                                        float* __restrict__ occl1, float* __restrict__ occl2,
                                                        int B, int H, int W, float dist_thresh, float wthresh) {
    const int64_t hw = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * hw) return;
    const int b = (int)(i / hw);
    const int64_t pix = i % hw;
    const int yy = (int)(pix / W), xx = (int)(pix % W);
    const float* m1 = mask1 + (int64_t)b * hw;
    const float* m2 = mask2 + (int64_t)b * hw;
    const float* f12 = flow12 + (int64_t)b * fbstride;
    const float* f21 = flow21 + (int64_t)b * fbstride;
    const float* s12 = scale12 ? scale12 + (int64_t)b * hw : nullptr;
    const float* s21 = scale21 ? scale21 + (int64_t)b * hw : nullptr;
    occl1[i] = occl_one(m1, m2, f12, f21, s12, s21, hw, H, W, xx, yy, dist_thresh, wthresh);
    occl2[i] = occl_one(m2, m1, f21, f12, s21, s12, hw, H, W, xx, yy, dist_thresh, wthresh);
}

// occlusion_kernel + flow_finalize_forward_kernel of both directions in one pass (mr_occlusion_flow): the pixel
// that has just computed its two occlusion bits also holds everything the final flows need --
// out12[b, y, x, c] = (flow12[b, c, y, x] * scale12) * (mask1 * occl1), likewise 21 -- inside the crop.
__global__ void __launch_bounds__(256) occlusion_flow_kernel(const float* __restrict__ mask1,
                                                             const float* __restrict__ mask2,
                                                             const float* __restrict__ flow12,
                                                             const float* __restrict__ flow21, int64_t fbstride,
                                                             const float* __restrict__ scale12,
                                                             const float* __restrict__ scale21,
                                                             float* __restrict__ occl1, float* __restrict__ occl2,
                                                             float* __restrict__ out12, float* __restrict__ out21,
                                                             int B, int H, int W, int crop_h, int crop_w,
                                                             float dist_thresh, float wthresh,
                                                             const uint8_t* __restrict__ hit1,
                                                             const uint8_t* __restrict__ hit2, int tiles_x,
                                                             int tiles_y) {
    const int64_t hw = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * hw) return;
    const int b = (int)(i / hw);
    const int64_t pix = i % hw;
    const int yy = (int)(pix / W), xx = (int)(pix % W);
    const float* m1 = mask1 + (int64_t)b * hw;
    const float* m2 = mask2 + (int64_t)b * hw;
    const float* f12 = flow12 + (int64_t)b * fbstride;
    const float* f21 = flow21 + (int64_t)b * fbstride;
    const float* s12 = scale12 ? scale12 + (int64_t)b * hw : nullptr;
    const float* s21 = scale21 ? scale21 + (int64_t)b * hw : nullptr;
    const uint8_t* h1 = hit1 ? hit1 + (int64_t)b * tiles_x * tiles_y * 4 : nullptr;
    const uint8_t* h2 = hit2 ? hit2 + (int64_t)b * tiles_x * tiles_y * 4 : nullptr;
    const float o1 = occl_one(m1, m2, f12, f21, s12, s21, hw, H, W, xx, yy, dist_thresh, wthresh, h1, h2, tiles_x);
    const float o2 = occl_one(m2, m1, f21, f12, s21, s12, hw, H, W, xx, yy, dist_thresh, wthresh, h2, h1, tiles_x);
    occl1[i] = o1;
    occl2[i] = o2;
    if (yy < crop_h && xx < crop_w) {
        const int64_t o = ((int64_t)b * crop_h + yy) * crop_w + xx;
        // (an occlusion bit can only be non-zero at a pixel inside its own image's coverage: the guarded reads of
        // occl_one came first)
        const float a1 = (o1 != 0.0f && s12) ? s12[pix] : 1.0f, a2 = (o2 != 0.0f && s21) ? s21[pix] : 1.0f;
        const float post1 = o1 != 0.0f ? m1[pix] * o1 : 0.0f, post2 = o2 != 0.0f ? m2[pix] * o2 : 0.0f;
        // (x * a) * 0 is a zero for the finite rendered values: not loaded where the masks are 0
        float2 r12 = make_float2(0.0f, 0.0f), r21 = make_float2(0.0f, 0.0f);
        if (post1 != 0.0f && a1 != 0.0f) r12 = make_float2((f12[pix] * a1) * post1, (f12[hw + pix] * a1) * post1);
        if (post2 != 0.0f && a2 != 0.0f) r21 = make_float2((f21[pix] * a2) * post2, (f21[hw + pix] * a2) * post2);
        *reinterpret_cast<float2*>(out12 + o * 2) = r12;
        *reinterpret_cast<float2*>(out21 + o * 2) = r21;
    }
}

// ---------------------------------------------------------------------------------------
// flow epilogue of opticalflow.get_opticalflow (opticalflow.py:109-154)
// ---------------------------------------------------------------------------------------
// mask[b, yi_img, x] = (alpha > thresh) * keep(face_index_map[b, is - 1 - yi_img, x])
// keep(f) = lut[f + 1] for f + 1 < n_lut, else 1 (lut[0] is the background slot)
__global__ void __launch_bounds__(256) flow_mask_kernel(const float* __restrict__ alpha,
                                                        const int32_t* __restrict__ fim,
                                                        const float* __restrict__ lut, int n_lut, float thresh,
                                                        float* __restrict__ mask, int64_t npx, int is) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    float m = (alpha[i] > thresh) ? 1.0f : 0.0f;
    if (lut) {
        const int64_t plane = (int64_t)is * is;
        const int64_t b = i / plane;
        const int pix = (int)(i % plane);
        const int yi = pix / is, xi = pix % is;
        const int f = fim[b * plane + (int64_t)(is - 1 - yi) * is + xi] + 1;
        m = m * ((f >= 0 && f < n_lut) ? lut[f] : 1.0f);
    }
    mask[i] = m;
}

// flow[b, y, x, c] = (rgb[b, c, y, x] * m_pre) * (m_x * occl), c = 0, 1, cropped to H x W
__global__ void __launch_bounds__(256) flow_finalize_forward_kernel(
    const float* __restrict__ rgb, const float* __restrict__ m_pre, const float* __restrict__ m_x,
    const float* __restrict__ occl, float* __restrict__ flow, int B, int is, int H, int W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * H * W) return;
    const int b = (int)(i / ((int64_t)H * W));
    const int pix = (int)(i % ((int64_t)H * W));
    const int y = pix / W, x = pix % W;
    const int64_t plane = (int64_t)is * is, o = (int64_t)b * plane + (int64_t)y * is + x;
    const float a = m_pre[o], post = m_x[o] * occl[o];
    const float r0 = rgb[(int64_t)b * 3 * plane + (int64_t)y * is + x], r1 = rgb[((int64_t)b * 3 + 1) * plane + (int64_t)y * is + x];
    *reinterpret_cast<float2*>(flow + i * 2) = make_float2((r0 * a) * post, (r1 * a) * post);
}

// grad_rgb[b, c, y, x] = grad_flow[b, y, x, c] * post * m_pre inside the crop, 0 elsewhere / for c = 2
__global__ void __launch_bounds__(256) flow_finalize_backward_kernel(
    const float* __restrict__ grad_flow, const float* __restrict__ m_pre, const float* __restrict__ m_x,
    const float* __restrict__ occl, float* __restrict__ grad_rgb, int B, int is, int H, int W) {
    const int64_t plane = (int64_t)is * is;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * plane) return;
    const int64_t b = i / plane;
    const int pix = (int)(i % plane);
    const int y = pix / is, x = pix % is;
    float g0 = 0.0f, g1 = 0.0f;
    if (y < H && x < W) {
        const float a = m_pre[i], post = m_x[i] * occl[i];
        const float2 g = *reinterpret_cast<const float2*>(grad_flow + ((b * H + y) * (int64_t)W + x) * 2);
        g0 = (g.x * post) * a;
        g1 = (g.y * post) * a;
    }
    grad_rgb[b * 3 * plane + pix] = g0;
    grad_rgb[(b * 3 + 1) * plane + pix] = g1;
    grad_rgb[(b * 3 + 2) * plane + pix] = 0.0f;
}

// ---------------------------------------------------------------------------------------
// pair_consist
// ---------------------------------------------------------------------------------------
struct PairParams {
    const float* flow12;  // [B,H,W,2]
    const float* flow21;
    const float* image_ref;  // [B,3,H,W]
    const float* image;
    const float* jitter_ref;  // [B,Cj,H,W]
    const float* jitter;
    int Cj;
    float* partial;  // [B, nblk, 4]
    uint8_t* full_mask1;
    uint8_t* full_mask2;
    float* warp_mask1;  // [B,3,H,W]
    float* warp_mask2;
    float* warp1;
    float* warp2;
    float* diff1;
    float* diff2;
    int B, H, W, nblk, tiles_x;
    float thresh;
    // optional coverage bytes of the renders the flows came from (mr_render_flow_forward): a flow is exactly 0
    // where its render covered nothing, and is not even read there
    const uint8_t* hit12;  // [B, tiles_y, tiles_x, 4] of the render behind flow12 (frame 1)
    const uint8_t* hit21;
    int hit_is, hit_tiles_x, hit_stride;  // raster size, tiles per raster row, bytes per image
};

// 64 x 4 pixel tiles (one 256-B row per wave); logical tile id -> (sample, tile) with the XCD-aware remap so that
// vertically adjacent tiles (which share bilinear taps) run behind the same L2.
constexpr int PT_W = 64, PT_H = 4;
// tiles per workgroup of the BACKWARD kernel: once most blocks leave early a launch is bound by its workgroup count (43
// instead of 46 us in the training step).  The forward, with its block reduction per tile, is slower that way (56 us).
constexpr int PT_SUB = 4;
__device__ __forceinline__ bool pair_tile_pixel(unsigned lid, int H, int W, int tiles_x, int ntiles, int& b, int& tile,
                                                int& xx, int& yy) {
    b = lid / ntiles;
    tile = lid % ntiles;
    xx = (tile % tiles_x) * PT_W + (threadIdx.x % PT_W);
    yy = (tile / tiles_x) * PT_H + (threadIdx.x / PT_W);
    return xx < W && yy < H;
}

// Does the render behind a flow cover anything in the block's PT_W x PT_H pixels?  Block-uniform (scalar loads of
// the 4-byte coverage words of the <= 3 x 2 raster tiles the block touches); NULL = no information = yes.
__device__ __forceinline__ bool pair_block_covered(const uint8_t* __restrict__ hit, int hit_is, int hit_tiles_x,
                                                   int hit_stride, int b, int tile, int tiles_x, int H, int W) {
    if (!hit) return true;
    const int x0 = (tile % tiles_x) * PT_W, y0 = (tile / tiles_x) * PT_H;
    const int x1 = min(x0 + PT_W, W) - 1, y1 = min(y0 + PT_H, H) - 1;
    const uint32_t* h32 = reinterpret_cast<const uint32_t*>(hit + (int64_t)b * hit_stride);
    uint32_t any = 0u;
    for (int ty = (hit_is - 1 - y1) >> 3; ty <= (hit_is - 1 - y0) >> 3; ty++)
        for (int tx = x0 >> 5; tx <= x1 >> 5; tx++) any |= h32[ty * hit_tiles_x + tx];
    return any != 0u;
}

// ... in either of two renders: the words of both are requested before any is looked at (one round trip, not two --
// five sixths of the blocks of a hand + object frame pair end here, and their number times this latency over the
// resident workgroups is the floor of the launch)
__device__ __forceinline__ bool pair_block_covered2(const uint8_t* __restrict__ hit_a, const uint8_t* __restrict__ hit_b,
                                                    int hit_is, int hit_tiles_x, int hit_stride, int b, int tile, int tiles_x,
                                                    int H, int W) {
    const int x0 = (tile % tiles_x) * PT_W, y0 = (tile / tiles_x) * PT_H;
    const int x1 = min(x0 + PT_W, W) - 1, y1 = min(y0 + PT_H, H) - 1;
    const uint32_t* a32 = reinterpret_cast<const uint32_t*>(hit_a + (int64_t)b * hit_stride);
    const uint32_t* b32 = reinterpret_cast<const uint32_t*>(hit_b + (int64_t)b * hit_stride);
    uint32_t any = 0u;
    for (int ty = (hit_is - 1 - y1) >> 3; ty <= (hit_is - 1 - y0) >> 3; ty++)
        for (int tx = x0 >> 5; tx <= x1 >> 5; tx++) any |= a32[ty * hit_tiles_x + tx] | b32[ty * hit_tiles_x + tx];
    return any != 0u;
}

template <PairCrit CRIT>
__device__ __forceinline__ void pair_consist_forward_body(const PairParams& p) {
    __shared__ float red[4][4];
    const int64_t hw = (int64_t)p.H * p.W;
    int b, tile, xx, yy;
    const bool in_img = pair_tile_pixel(xcd_remap(blockIdx.x, gridDim.x), p.H, p.W, p.tiles_x, p.nblk, b, tile, xx, yy);
    // nothing rendered under this block in either frame: both flows are zero here, no pixel is valid -- the block's
    // partial sums are zero (no loads, no barrier), unless the per-pixel debug outputs want every pixel
    if (p.hit12 && p.hit21 && !(p.warp1 || p.warp2 || p.diff1 || p.diff2 || p.warp_mask1 || p.warp_mask2 ||
                                p.full_mask1 || p.full_mask2) &&
        !pair_block_covered2(p.hit12, p.hit21, p.hit_is, p.hit_tiles_x, p.hit_stride, b, tile, p.tiles_x, p.H, p.W)) {
        if (threadIdx.x < 4) p.partial[((int64_t)b * p.nblk + tile) * 4 + threadIdx.x] = 0.0f;
        return;
    }
    float sum1 = 0.0f, cnt1 = 0.0f, sum2 = 0.0f, cnt2 = 0.0f;
    if (in_img) {
        const int64_t pix = (int64_t)yy * p.W + xx;
        const bool allj = p.warp_mask1 != nullptr || p.warp_mask2 != nullptr;
        // forward term: image_ref warped by flow21 vs image (imgflowarp.py:80,85-87,93-102)
        // backward term: image warped by flow12 vs image_ref (:84,82,88,99-107)
        const float2 uv1 = pair_flow(p.flow21, p.hit21, p.hit_is, p.hit_tiles_x, p.hit_stride, b, xx, yy, p.H, p.W);
        const float2 uv2 = pair_flow(p.flow12, p.hit12, p.hit_is, p.hit_tiles_x, p.hit_stride, b, xx, yy, p.H, p.W);
        // A pixel whose flow has a zero x component is invalid whatever the images hold (imgflowarp.py:93-100,
        // SURVEY Q5) and adds nothing to the masked sums: unless the per-pixel outputs (warps, differences,
        // warp masks) are requested, neither its taps are computed nor its 26 tap loads issued -- a rendered flow is
        // exactly 0 outside the meshes, 90 % of a hand + object frame.
        const bool per_pixel_out = p.warp1 || p.warp2 || p.diff1 || p.diff2 || p.warp_mask1 || p.warp_mask2;
        const bool need1 = per_pixel_out || uv1.x != 0.0f, need2 = per_pixel_out || uv2.x != 0.0f;
        DirTaps t1{}, t2{};
        if (need1) t1 = pair_taps(uv1, xx, yy, p.H, p.W);
        if (need2) t2 = pair_taps(uv2, xx, yy, p.H, p.W);
        DirRaw2 q1{}, q2{};
        if (need1) pair_load(t1, p.image_ref, p.image, p.jitter, p.jitter, p.Cj, allj, b, pix, hw, q1);
        if (need2) pair_load(t2, p.image, p.image_ref, p.jitter_ref, p.jitter_ref, p.Cj, allj, b, pix, hw, q2);
        pin(q1); pin(q2);
        const DirRaw r1 = unpack(q1, t1.a), r2 = unpack(q2, t2.a);
        DirOut d1{}, d2{};
        if (need1) d1 = pair_eval(t1, r1, p.H, p.W, p.thresh, allj && p.Cj == 3);
        if (need2) d2 = pair_eval(t2, r2, p.H, p.W, p.thresh, allj && p.Cj == 3);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int64_t o = ((int64_t)b * 3 + c) * hw + pix;
            const float df = pair_term<CRIT>(d1.s[c] - r1.tgt[c]);
            const float db = pair_term<CRIT>(d2.s[c] - r2.tgt[c]);
            if (d1.valid) sum1 += df;
            if (d2.valid) sum2 += db;
            if (p.warp1) p.warp1[o] = d1.s[c];
            if (p.warp2) p.warp2[o] = d2.s[c];
            if (p.diff1) p.diff1[o] = df;
            if (p.diff2) p.diff2[o] = db;
            if (p.warp_mask1) p.warp_mask1[o] = d1.wm[c];
            if (p.warp_mask2) p.warp_mask2[o] = d2.wm[c];
        }
        if (d1.valid) cnt1 = 3.0f;
        if (d2.valid) cnt2 = 3.0f;
        if (p.full_mask1) p.full_mask1[(int64_t)b * hw + pix] = d1.valid ? 1 : 0;
        if (p.full_mask2) p.full_mask2[(int64_t)b * hw + pix] = d2.valid ? 1 : 0;
    }
    float v[4] = {sum1, cnt1, sum2, cnt2};
    block_sum4(v, red);
    if (threadIdx.x == 0) {
        float* o = p.partial + ((int64_t)b * p.nblk + tile) * 4;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    }
}

// per-sample fixed-order reduction of the block partials -> sums[B,4], loss_fwd/bwd[B]
__global__ void __launch_bounds__(64) pair_consist_finalize_kernel(const float* __restrict__ partial, int nblk,
                                                                   float* __restrict__ sums,
                                                                   float* __restrict__ loss_fwd,
                                                                   float* __restrict__ loss_bwd) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = lane; j < nblk; j += 64) {
        const float4 v = *reinterpret_cast<const float4*>(partial + ((int64_t)b * nblk + j) * 4);
        a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 4; k++) a[k] += __shfl_xor(a[k], off);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) sums[b * 4 + k] = a[k];
        const float n1 = (a[1] == 0.0f) ? 1.0f : a[1], n2 = (a[3] == 0.0f) ? 1.0f : a[3];
        if (loss_fwd) loss_fwd[b] = a[0] / n1;
        if (loss_bwd) loss_bwd[b] = a[2] / n2;
    }
}

struct PairBwdParams {
    const float* flow12;
    const float* flow21;
    const float* image_ref;
    const float* image;
    const float* jitter_ref;
    const float* jitter;
    int Cj;
    const float* sums;  // [B,4]
    const float* grad_loss_fwd;
    const float* grad_loss_bwd;  // nullable
    float* grad_flow12;
    float* grad_flow21;
    int B, H, W, ntiles, tiles_x;
    float thresh;
    const uint8_t* hit12;  // see PairParams
    const uint8_t* hit21;
    int hit_is, hit_tiles_x, hit_stride;
    unsigned* grad_max;    // nullable: [2B] float bits, zero on entry: max |grad_flow12[b]| at [b], |grad_flow21[b]| at [B + b]
};

template <PairCrit CRIT>
__device__ __forceinline__ void pair_consist_backward_body(const PairBwdParams& p) {
    const int64_t hw = (int64_t)p.H * p.W;
    const unsigned total = (unsigned)p.ntiles * (unsigned)p.B;
    const unsigned lid0 = xcd_remap(blockIdx.x, gridDim.x) * PT_SUB;
#pragma unroll 1
    for (unsigned lid = lid0; lid < min(lid0 + PT_SUB, total); lid++) {
    unsigned u12 = 0u, u21 = 0u;  // |gradient| of this thread's pixel as float bits (NaN > Inf > finite: a plain unsigned max)
    [&] {
    int b, tile, xx, yy;
    if (!pair_tile_pixel(lid, p.H, p.W, p.tiles_x, p.ntiles, b, tile, xx, yy)) return;
    const int64_t pix = (int64_t)yy * p.W + xx;
    if (p.hit12 && p.hit21 &&
        !pair_block_covered2(p.hit12, p.hit21, p.hit_is, p.hit_tiles_x, p.hit_stride, b, tile, p.tiles_x, p.H, p.W)) {
        // nothing rendered under this block in either frame: zero gradient, nothing read
        *reinterpret_cast<float2*>(p.grad_flow21 + ((int64_t)b * hw + pix) * 2) = make_float2(0.0f, 0.0f);
        *reinterpret_cast<float2*>(p.grad_flow12 + ((int64_t)b * hw + pix) * 2) = make_float2(0.0f, 0.0f);
        return;
    }
    const float c1 = p.sums[b * 4 + 1], c2 = p.sums[b * 4 + 3];
    const float coef1 = pair_coef(p.grad_loss_fwd[b], c1);
    const float coef2 = p.grad_loss_bwd ? pair_coef(p.grad_loss_bwd[b], c2) : 0.0f;
    const bool both = p.grad_loss_bwd != nullptr;
    const float2 uv1 = pair_flow(p.flow21, p.hit21, p.hit_is, p.hit_tiles_x, p.hit_stride, b, xx, yy, p.H, p.W);
    const float2 uv2 = both ? pair_flow(p.flow12, p.hit12, p.hit_is, p.hit_tiles_x, p.hit_stride, b, xx, yy, p.H, p.W) : uv1;
    // the gradient of an invalid pixel is 0: no taps, no tap loads where the flow's x component is zero (see the
    // forward kernel)
    const bool need1 = uv1.x != 0.0f && coef1 != 0.0f, need2 = both && uv2.x != 0.0f && coef2 != 0.0f;
    DirTaps t1{}, t2{};
    if (need1) t1 = pair_taps(uv1, xx, yy, p.H, p.W);
    if (need2) t2 = pair_taps(uv2, xx, yy, p.H, p.W);
    DirRaw2 q1{}, q2{};
    if (need1) pair_load(t1, p.image_ref, p.image, p.jitter, p.jitter, p.Cj, false, b, pix, hw, q1);
    if (need2) pair_load(t2, p.image, p.image_ref, p.jitter_ref, p.jitter_ref, p.Cj, false, b, pix, hw, q2);
    pin(q1); pin(q2);
    float2 g21 = make_float2(0.0f, 0.0f), g12 = make_float2(0.0f, 0.0f);
    if (need1) {
        const DirRaw r1 = unpack(q1, t1.a);
        const DirOut d1 = pair_eval(t1, r1, p.H, p.W, p.thresh, false);
        g21 = pair_grad<CRIT>(t1, r1, d1, p.H, p.W, coef1);
    }
    if (need2) {
        const DirRaw r2 = unpack(q2, t2.a);
        const DirOut d2 = pair_eval(t2, r2, p.H, p.W, p.thresh, false);
        g12 = pair_grad<CRIT>(t2, r2, d2, p.H, p.W, coef2);
    }
    *reinterpret_cast<float2*>(p.grad_flow21 + ((int64_t)b * hw + pix) * 2) = g21;
    *reinterpret_cast<float2*>(p.grad_flow12 + ((int64_t)b * hw + pix) * 2) = g12;
    u12 = abs_bits_max(g12);
    u21 = abs_bits_max(g21);
    }();
    // the largest |gradient| per image and direction, for the consumer of these gradients that scales them into fixed
    // point (mr_render_flow_backward's grad_bound: it saves that kernel a pass over its inputs).  Wave maximum at a
    // converged point, then one atomic per wave and direction -- and only while it still raises the stored value
    // (nine tenths of a rendered frame's pixels have a zero gradient).
    if (p.grad_max && __ballot((u12 | u21) != 0u) != 0ull) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            u12 = max(u12, (unsigned)__shfl_xor((int)u12, off));
            u21 = max(u21, (unsigned)__shfl_xor((int)u21, off));
        }
        if ((threadIdx.x & 63) == 0) {
            const unsigned b = lid / (unsigned)p.ntiles;
            if (u12 > p.grad_max[b]) atomicMax(&p.grad_max[b], u12);
            if (u21 > p.grad_max[p.B + b]) atomicMax(&p.grad_max[p.B + b], u21);
        }
    }
    }
}


// The kernels: one __global__ per criterion around each body (the l1 kernels keep their names -- profiles and the bench
// find them by name --, the l2 ones carry _l2); the host picks one per launch (MR_CRITERION_*).
__global__ void __launch_bounds__(256, 6) pair_consist_forward_kernel(PairParams p) { pair_consist_forward_body<PairCrit::L1>(p); }
__global__ void __launch_bounds__(256, 6) pair_consist_forward_l2_kernel(PairParams p) { pair_consist_forward_body<PairCrit::L2>(p); }
__global__ void __launch_bounds__(256) pair_consist_backward_kernel(PairBwdParams p) { pair_consist_backward_body<PairCrit::L1>(p); }
__global__ void __launch_bounds__(256) pair_consist_backward_l2_kernel(PairBwdParams p) { pair_consist_backward_body<PairCrit::L2>(p); }

}  // namespace mr

using namespace mr;

extern "C" int mr_warp_forward(const float* x, const float* flow, float* out, float* mask, int batch_size,
                               int channels, int height, int width, float thresh, int mode,
                               mr_stream_t stream) {
    if (!x || !flow || !out || !mask) return MR_ERR_BADARG;
    if (batch_size < 0 || channels < 0 || height <= 0 || width <= 0 || (mode != 0 && mode != 1))
        return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * height * width;
    if (channels == 0) return MR_OK;
    return launch1d(warp_forward_kernel, n, (hipStream_t)stream, x, flow, out, mask, batch_size, channels, height, width,
                    thresh, mode);
}

extern "C" int mr_warp_backward(const float* x, const float* flow, const float* grad_out, float* grad_x,
                                float* grad_flow, int batch_size, int channels, int height, int width,
                                float thresh, int mode, mr_stream_t stream) {
    if (!x || !flow || !grad_out) return MR_ERR_BADARG;
    if (batch_size < 0 || channels < 0 || height <= 0 || width <= 0 || (mode != 0 && mode != 1))
        return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * height * width;
    if (!grad_x && !grad_flow) return MR_OK;
    return launch1d(warp_backward_kernel, n, (hipStream_t)stream, x, flow, grad_out, grad_x, grad_flow, batch_size, channels,
                    height, width, thresh, mode);
}

extern "C" int mr_occlusion_mask(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                 const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                 const float* flow21_scale, float* occl1, float* occl2, int batch_size,
                                 int height, int width, float distance_thresh, float warp_thresh,
                                 mr_stream_t stream) {
    if (!mask_flow1 || !mask_flow2 || !flow12 || !flow21 || !occl1 || !occl2) return MR_ERR_BADARG;
    if (batch_size < 0 || height <= 0 || width <= 0 || flow_bstride < 2LL * height * width) return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * height * width;
    return launch1d(occlusion_kernel, n, (hipStream_t)stream, mask_flow1, mask_flow2, flow12, flow21, flow_bstride,
                    flow12_scale, flow21_scale, occl1, occl2, batch_size, height, width, distance_thresh, warp_thresh);
}

extern "C" int mr_occlusion_flow(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                 const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                 const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                 float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2, int batch_size,
                                 int height, int width, int crop_height, int crop_width, float distance_thresh,
                                 float warp_thresh, mr_stream_t stream) {
    if (!mask_flow1 || !mask_flow2 || !flow12 || !flow21 || !occl1 || !occl2 || !flow_out12 || !flow_out21)
        return MR_ERR_BADARG;
    if ((tile_hit1 == nullptr) != (tile_hit2 == nullptr) || (tile_hit1 && height != width)) return MR_ERR_BADARG;
    if (batch_size < 0 || height <= 0 || width <= 0 || flow_bstride < 2LL * height * width) return MR_ERR_BADARG;
    if (crop_height <= 0 || crop_width <= 0 || crop_height > height || crop_width > width) return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * height * width;
    return launch1d(occlusion_flow_kernel, n, (hipStream_t)stream, mask_flow1, mask_flow2, flow12, flow21, flow_bstride,
                    flow12_scale, flow21_scale, occl1, occl2, flow_out12, flow_out21, batch_size, height, width, crop_height,
                    crop_width, distance_thresh, warp_thresh, tile_hit1, tile_hit2, (width + 31) / 32, (height + 7) / 8);
}

extern "C" int64_t mr_pair_consist_workspace_bytes(int batch_size, int height, int width) {
    if (batch_size < 0 || height <= 0 || width <= 0) return MR_ERR_BADARG;
    // ONE region at the base: four partial sums per 64 x 4 tile
    const int64_t nblk = (int64_t)((width + PT_W - 1) / PT_W) * ((height + PT_H - 1) / PT_H);
    return (int64_t)batch_size * nblk * 4 * (int64_t)sizeof(float);
}

// What mr_pair_consist_forward_crit and _backward_crit share: the argument checks (`ptrs_ok`: the caller's own pointers and
// workspace; every refusal is MR_ERR_BADARG, so their order does not show) and the tile arithmetic of the launch.
struct PairGrid {
    int tiles_x, nblk;             // 64 x 4 pixel tiles per row / per image
    int hit_tiles_x, hit_stride;   // coverage bytes: tiles per raster row, bytes per image
};
static int pair_consist_grid(bool ptrs_ok, int criterion, int jitter_channels, int batch_size, int height, int width, bool has_hit,
                             int hit_image_size, PairGrid& g) {
    if (!criterion_ok(criterion) || !ptrs_ok) return MR_ERR_BADARG;
    if (has_hit && (hit_image_size < height || hit_image_size < width)) return MR_ERR_BADARG;
    if (jitter_channels != 1 && jitter_channels != 3) return MR_ERR_BADARG;
    if (batch_size < 0 || height <= 0 || width <= 0) return MR_ERR_BADARG;
    if (width < 2 || (int64_t)height * width > (1LL << 29)) return MR_ERR_BADARG;  // row-pair taps, 32-bit byte offsets
    g.tiles_x = (width + PT_W - 1) / PT_W;
    g.nblk = g.tiles_x * ((height + PT_H - 1) / PT_H);
    if (!grid_ok((int64_t)g.nblk * batch_size)) return MR_ERR_BADARG;
    g.hit_tiles_x = (hit_image_size + 31) / 32;
    g.hit_stride = g.hit_tiles_x * ((hit_image_size + 7) / 8) * 4;
    return MR_OK;
}

extern "C" int mr_pair_consist_forward_crit(const float* flow12, const float* flow21, const float* image_ref,
                                            const float* image, const float* jitter_ref, const float* jitter,
                                            int jitter_channels, void* workspace, int64_t workspace_bytes,
                                            float* sums, float* loss_fwd, float* loss_bwd, uint8_t* full_mask1,
                                            uint8_t* full_mask2, float* warp_mask1, float* warp_mask2,
                                            float* warp1, float* warp2, float* diff1, float* diff2,
                                            int batch_size, int height, int width, float thresh,
                                            const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                                            mr_stream_t stream, int criterion) {
    PairGrid g;
    const int rc = pair_consist_grid(flow12 && flow21 && image_ref && image && jitter_ref && jitter && workspace && sums &&
                                         workspace_bytes >= mr_pair_consist_workspace_bytes(batch_size, height, width),
                                     criterion, jitter_channels, batch_size, height, width, tile_hit12 || tile_hit21, hit_image_size, g);
    if (rc != MR_OK || batch_size == 0) return rc;
    const int nblk = g.nblk;
    PairParams p{};  // (value-initialised, then filled: the padding bytes are kernel-argument bytes too)
    p.flow12 = flow12; p.flow21 = flow21; p.image_ref = image_ref; p.image = image; p.jitter_ref = jitter_ref; p.jitter = jitter;
    p.Cj = jitter_channels; p.partial = (float*)workspace;
    p.full_mask1 = full_mask1; p.full_mask2 = full_mask2; p.warp_mask1 = warp_mask1; p.warp_mask2 = warp_mask2;
    p.warp1 = warp1; p.warp2 = warp2; p.diff1 = diff1; p.diff2 = diff2;
    p.B = batch_size; p.H = height; p.W = width; p.nblk = nblk; p.tiles_x = g.tiles_x; p.thresh = thresh;
    p.hit12 = tile_hit12; p.hit21 = tile_hit21; p.hit_is = hit_image_size; p.hit_tiles_x = g.hit_tiles_x; p.hit_stride = g.hit_stride;
    hipLaunchKernelGGL(criterion == MR_CRITERION_L2 ? pair_consist_forward_l2_kernel : pair_consist_forward_kernel,
                       dim3((unsigned)(nblk * batch_size)), dim3(256), 0, (hipStream_t)stream, p);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(pair_consist_finalize_kernel, dim3(batch_size), dim3(64), 0, (hipStream_t)stream,
                       (const float*)workspace, nblk, sums, loss_fwd, loss_bwd);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_pair_consist_forward(const float* flow12, const float* flow21, const float* image_ref,
                                       const float* image, const float* jitter_ref, const float* jitter,
                                       int jitter_channels, void* workspace, int64_t workspace_bytes,
                                       float* sums, float* loss_fwd, float* loss_bwd, uint8_t* full_mask1,
                                       uint8_t* full_mask2, float* warp_mask1, float* warp_mask2,
                                       float* warp1, float* warp2, float* diff1, float* diff2,
                                       int batch_size, int height, int width, float thresh,
                                       const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                                       mr_stream_t stream) {
    return mr_pair_consist_forward_crit(flow12, flow21, image_ref, image, jitter_ref, jitter, jitter_channels, workspace,
                                        workspace_bytes, sums, loss_fwd, loss_bwd, full_mask1, full_mask2, warp_mask1, warp_mask2,
                                        warp1, warp2, diff1, diff2, batch_size, height, width, thresh, tile_hit12, tile_hit21,
                                        hit_image_size, stream, MR_CRITERION_L1);
}

extern "C" int mr_pair_consist_backward_crit(const float* flow12, const float* flow21, const float* image_ref,
                                             const float* image, const float* jitter_ref, const float* jitter,
                                             int jitter_channels, const float* sums, const float* grad_loss_fwd,
                                             const float* grad_loss_bwd, float* grad_flow12, float* grad_flow21,
                                             int batch_size, int height, int width, float thresh,
                                             const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                                             float* grad_max, mr_stream_t stream, int criterion) {
    PairGrid g;
    const int rc = pair_consist_grid(flow12 && flow21 && image_ref && image && jitter_ref && jitter && sums && grad_loss_fwd &&
                                         grad_flow12 && grad_flow21,
                                     criterion, jitter_channels, batch_size, height, width, tile_hit12 || tile_hit21, hit_image_size, g);
    if (rc != MR_OK || batch_size == 0) return rc;
    const int nblk = g.nblk;
    PairBwdParams p{};  // (value-initialised, then filled: see mr_pair_consist_forward_crit)
    p.flow12 = flow12; p.flow21 = flow21; p.image_ref = image_ref; p.image = image; p.jitter_ref = jitter_ref; p.jitter = jitter;
    p.Cj = jitter_channels; p.sums = sums; p.grad_loss_fwd = grad_loss_fwd; p.grad_loss_bwd = grad_loss_bwd;
    p.grad_flow12 = grad_flow12; p.grad_flow21 = grad_flow21;
    p.B = batch_size; p.H = height; p.W = width; p.ntiles = nblk; p.tiles_x = g.tiles_x; p.thresh = thresh;
    p.hit12 = tile_hit12; p.hit21 = tile_hit21; p.hit_is = hit_image_size; p.hit_tiles_x = g.hit_tiles_x; p.hit_stride = g.hit_stride;
    p.grad_max = reinterpret_cast<unsigned*>(grad_max);
    hipLaunchKernelGGL(criterion == MR_CRITERION_L2 ? pair_consist_backward_l2_kernel : pair_consist_backward_kernel,
                       dim3((unsigned)((nblk * batch_size + PT_SUB - 1) / PT_SUB)), dim3(256), 0, (hipStream_t)stream, p);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_pair_consist_backward(const float* flow12, const float* flow21, const float* image_ref,
                                        const float* image, const float* jitter_ref, const float* jitter,
                                        int jitter_channels, const float* sums, const float* grad_loss_fwd,
                                        const float* grad_loss_bwd, float* grad_flow12, float* grad_flow21,
                                        int batch_size, int height, int width, float thresh,
                                        const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                                        float* grad_max, mr_stream_t stream) {
    return mr_pair_consist_backward_crit(flow12, flow21, image_ref, image, jitter_ref, jitter, jitter_channels, sums,
                                         grad_loss_fwd, grad_loss_bwd, grad_flow12, grad_flow21, batch_size, height, width,
                                         thresh, tile_hit12, tile_hit21, hit_image_size, grad_max, stream, MR_CRITERION_L1);
}

extern "C" int mr_flow_mask(const float* alpha_img, const int32_t* face_index_map, const float* keep_lut, int n_lut,
                            float thresh, float* mask, int batch_size, int image_size, mr_stream_t stream) {
    if (!alpha_img || !mask || batch_size < 0 || image_size <= 0) return MR_ERR_BADARG;
    if (keep_lut && (!face_index_map || n_lut <= 0)) return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * image_size * image_size;
    return launch1d(flow_mask_kernel, n, (hipStream_t)stream, alpha_img, face_index_map, keep_lut, n_lut, thresh, mask, n,
                    image_size);
}

extern "C" int mr_flow_finalize_forward(const float* rgb_img, const float* mask_pre, const float* mask_x,
                                        const float* occl, float* flow, int batch_size, int image_size, int height,
                                        int width, mr_stream_t stream) {
    if (!rgb_img || !mask_pre || !mask_x || !occl || !flow) return MR_ERR_BADARG;
    if (batch_size < 0 || image_size <= 0 || height <= 0 || width <= 0 || height > image_size || width > image_size)
        return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * height * width;
    return launch1d(flow_finalize_forward_kernel, n, (hipStream_t)stream, rgb_img, mask_pre, mask_x, occl, flow, batch_size,
                    image_size, height, width);
}

extern "C" int mr_flow_finalize_backward(const float* grad_flow, const float* mask_pre, const float* mask_x,
                                         const float* occl, float* grad_rgb_img, int batch_size, int image_size,
                                         int height, int width, mr_stream_t stream) {
    if (!grad_flow || !mask_pre || !mask_x || !occl || !grad_rgb_img) return MR_ERR_BADARG;
    if (batch_size < 0 || image_size <= 0 || height <= 0 || width <= 0 || height > image_size || width > image_size)
        return MR_ERR_BADARG;
    const int64_t n = (int64_t)batch_size * image_size * image_size;
    return launch1d(flow_finalize_backward_kernel, n, (hipStream_t)stream, grad_flow, mask_pre, mask_x, occl, grad_rgb_img,
                    batch_size, image_size, height, width);
}
