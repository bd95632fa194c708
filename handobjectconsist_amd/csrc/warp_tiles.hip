// warp_tiles.hip -- photometric warp kernels for gfx950 (MI355X), the listed launches of the training path: occlusion,
// flow epilogue and pair loss over the stacked render's tile list, one list entry per workgroup (see "Listed launches"
// below).  The dense launches are in warp.hip; the device functions both use (sampling, the pair criterion, block_sum4,
// tile_at) are in warp_device.hpp.
//
// Kernels, in file order: occlusion_flow_tiles_kernel, pair_consist_finalize_tiles_kernel,
// pair_consist_forward_tiles_kernel, pair_consist_forward_tiles_l2_kernel, pair_consist_backward_tiles_kernel,
// pair_consist_backward_tiles_l2_kernel, and the fused forward of the pair step flow_pair_forward_tiles_kernel<GRAD, REC>
// with its _l2, _bf16u8, _l2_bf16u8, _bf16f32 and _l2_bf16f32 forms (criterion x element types of the image batch).
//
// Entry points: mr_occlusion_flow_tiles, mr_pair_consist_tiles_workspace_bytes, mr_flow_pair_scatter_work_bytes,
// mr_pair_consist_forward_tiles[_crit], mr_pair_consist_backward_tiles[_crit], mr_flow_pair_forward_grad_tiles[_crit|_typed],
// mr_flow_pair_forward_tiles[_crit|_typed], and mr::launch_flow_pair_forward for pair_step.hip.
#include <algorithm>

#include "mr_common.hpp"
#include "pair_launch.hpp"
#include "warp_device.hpp"

namespace mr {

// ---------------------------------------------------------------------------------------
// Listed launches (mr_*_tiles): the warp half of the training path over the render's tile list
// ---------------------------------------------------------------------------------------
// A frame pair's hand + object meshes cover a sixth of the screen.  The dense kernels above launch a workgroup for
// every block of every image (16 384 of them at B = 64, 256 x 256), five sixths of which read their coverage words and
// leave -- residency x lifetime of those workgroups is half of the dense launch (27 / 23 / 21 us of 47 / 45 / 39), and
// the epilogue and the pair backward still WRITE their zeros under them (98 + 66 MB per step, for no reader: every
// consumer on the training path consults the coverage bytes first).  The render of the stacked pair (2B images: frame
// 1 of every pair, then frame 2) already holds the list of the tiles with candidate faces (raster_fwd.hip:
// bin_boxes_kernel); everything the warp half computes about direction 1 -> 2 lives at pixels frame 1's render covers
// (occl1, flow12, the pair loss's backward term, grad_flow12), and likewise for 2 -> 1 -- so ONE list entry (image of
// the stack, 32 x 8 raster tile) is one workgroup's work in all three kernels, one pixel per thread, and nothing is
// dispatched, read or written for the rest of the screen.  Granularity of the contract: a tile whose 4-byte coverage
// word is non-zero gets all its pixels (inside the crop) written; tiles with a zero word -- listed or not -- get
// NOTHING, and no reader may use what it finds there (round 6: the fused forward reads a value next to the byte that guards it
// and drops it by a select -- addresses inside the planes, contents never used).  Same XCD slices as the render's tile kernel (list_slice): what it wrote for
// a tile is read back behind the same L2.
struct OcclTilesParams {
    const float* mask[2];    // mask_flow1 / mask_flow2  [B,is,is]
    const float* flow[2];    // flow12 / flow21 planes (batch stride fbstride)
    const float* scale[2];   // nullable
    float* occl[2];
    float* out[2];           // [B,crop_h,crop_w,2]
    const uint8_t* hit[2];
    int64_t fbstride;
    int B, is, crop_h, crop_w, tiles_x, tiles_y;
    float dist_thresh, wthresh;
    ListArgs list;
};

__global__ void __launch_bounds__(256) occlusion_flow_tiles_kernel(OcclTilesParams p) {
    unsigned j;
    const ListSlice sl = list_slice(p.list.tlist->n_heavy, p.list.tlist->n_light, j);
    const int T = p.tiles_x * p.tiles_y, is = p.is;
    const int64_t hw = (int64_t)is * is;
    for (; j < sl.n_local; j += sl.stride) {
        const TileAt t = tile_at(p.list.ids[sl.slot(j, p.list.cap)].x, p.B, p.tiles_x, T, is, p.hit[0], p.hit[1]);
        if (t.word == 0u || t.x >= is || t.ry >= is) continue;  // (uniform | border tiles of rasters that are no multiple of the tile)
        const int a = t.dir, o_ = 1 - t.dir;
        const float* ma = p.mask[a] + (int64_t)t.b * hw;
        const float* mb = p.mask[o_] + (int64_t)t.b * hw;
        const float* fab = p.flow[a] + (int64_t)t.b * p.fbstride;
        const float* fba = p.flow[o_] + (int64_t)t.b * p.fbstride;
        const float* sab = p.scale[a] ? p.scale[a] + (int64_t)t.b * hw : nullptr;
        const float* sba = p.scale[o_] ? p.scale[o_] + (int64_t)t.b * hw : nullptr;
        const uint8_t* ha = p.hit[a] + (int64_t)t.b * T * 4;
        const uint8_t* hb = p.hit[o_] + (int64_t)t.b * T * 4;
        const int64_t pix = (int64_t)t.y * is + t.x;
        float o = 0.0f;
        if (t.row_covered) o = occl_one(ma, mb, fab, fba, sab, sba, hw, is, is, t.x, t.y, p.dist_thresh, p.wthresh, ha, hb, p.tiles_x);
        p.occl[a][(int64_t)t.b * hw + pix] = o;
        if (t.y < p.crop_h && t.x < p.crop_w) {
            // (an occlusion bit can only be non-zero inside its own image's coverage: occl_one's guarded reads came first)
            const float sc = (o != 0.0f && sab) ? sab[pix] : 1.0f;
            const float post = o != 0.0f ? ma[pix] * o : 0.0f;
            float2 r = make_float2(0.0f, 0.0f);
            if (post != 0.0f && sc != 0.0f) r = make_float2((fab[pix] * sc) * post, (fab[hw + pix] * sc) * post);
            *reinterpret_cast<float2*>(p.out[a] + (((int64_t)t.b * p.crop_h + t.y) * p.crop_w + t.x) * 2) = r;
        }
    }
}

struct PairTilesParams {
    const float* flow[2];     // flow12 / flow21 [B,H,W,2]
    const float* image_ref;   // [B,3,H,W]
    const float* image;
    const float* jitter_ref;  // [B,Cj,H,W]
    const float* jitter;
    int Cj;
    float* partial;           // forward: [2B, T, 2] {masked L1 sum, 3 x valid count} of stack image i's direction
    const uint8_t* hit[2];
    int B, H, W, is, tiles_x, tiles_y;
    float thresh;
    ListArgs list;
    // backward
    const float* sums;        // [B,4]
    const float* grad_loss_fwd;
    const float* grad_loss_bwd;  // nullable
    float* grad_flow[2];
    unsigned* grad_max;       // nullable, [2B]
};

// direction 0 = frame 1's pixel grid: flow12 warps `image` towards image_ref, gated by jitter_ref (imgflowarp.py:84,82,88,
// 99-107: the loss's "backward" term, sums[2..3]); direction 1 = frame 2's grid: flow21 warps image_ref towards image,
// gated by jitter (:80,85-87,93-102: the "forward" term, sums[0..1])
struct PairDir {
    const float* src;
    const float* tgt;
    const float* jit;
};
__device__ __forceinline__ PairDir pair_dir(const PairTilesParams& p, int dir) {
    PairDir d;
    d.src = dir ? p.image_ref : p.image;
    d.tgt = dir ? p.image : p.image_ref;
    d.jit = dir ? p.jitter : p.jitter_ref;
    return d;
}

template <PairCrit CRIT>
__device__ __forceinline__ void pair_consist_forward_tiles_body(const PairTilesParams& p) {
    __shared__ float red[2][4][2];
    unsigned j;
    const ListSlice sl = list_slice(p.list.tlist->n_heavy, p.list.tlist->n_light, j);
    const int T = p.tiles_x * p.tiles_y;
    const int64_t hw = (int64_t)p.H * p.W;
    unsigned round = 0;
    for (; j < sl.n_local; j += sl.stride) {
        const TileAt t = tile_at(p.list.ids[sl.slot(j, p.list.cap)].x, p.B, p.tiles_x, T, p.is, p.hit[0], p.hit[1]);
        if (t.word == 0u) continue;
        float sum = 0.0f, cnt = 0.0f;
        if (t.row_covered && t.x < p.W && t.y >= 0 && t.y < p.H) {
            const int64_t pix = (int64_t)t.y * p.W + t.x;
            const float2 uv = pair_flow(p.flow[t.dir], t.b, t.x, t.y, p.H, p.W);
            // a pixel whose flow has a zero x component is invalid whatever the images hold (imgflowarp.py:93-100)
            if (uv.x != 0.0f) {
                const PairDir d = pair_dir(p, t.dir);
                const DirPixel px = pair_pixel(uv, t.x, t.y, p.H, p.W, d.src, d.tgt, d.jit, p.Cj, t.b, pix, hw, p.thresh);
                if (px.e.valid) {
#pragma unroll
                    for (int c = 0; c < 3; c++) sum += pair_term<CRIT>(px.e.s[c] - px.r.tgt[c]);
                    cnt = 3.0f;
                }
            }
        }
        // block sums, fixed order (wave butterflies, then the four wave partials in wave order); the LDS slots alternate
        // between rounds so that a round needs ONE barrier
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { sum += __shfl_xor(sum, off); cnt += __shfl_xor(cnt, off); }
        // (`round` counts EXECUTED rounds -- tiles with a zero coverage word `continue` above: two consecutive executed rounds
        // must not share a slot, or a wave of the next round could overwrite it while thread 0 still reads)
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = round++ & 1u;
        if (lane == 0) { red[slot][wave][0] = sum; red[slot][wave][1] = cnt; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float* o = p.partial + ((int64_t)t.img * T + t.tile) * 2;
            o[0] = red[slot][0][0] + red[slot][1][0] + red[slot][2][0] + red[slot][3][0];
            o[1] = red[slot][0][1] + red[slot][1][1] + red[slot][2][1] + red[slot][3][1];
        }
    }
}

// occlusion_flow_tiles_kernel + pair_consist_forward_tiles_kernel in ONE pass (mr_flow_pair_forward_tiles): the thread that
// has just formed its pixel's final flow is the one that warps the image with it.  Same arithmetic, same per-tile partial
// sums (bit-identical losses); what disappears is the second kernel's chain of dependent loads (list counters -> entry ->
// coverage word -> flow) in front of its taps, and a launch.  The pixel's own image values (target, direct jitter) do
// not depend on the flow: they are requested before the occlusion check's gathers and have arrived when the taps go out.
struct FlowPairFwdParams {
    OcclTilesParams o;
    // (elements of the kernel's image type IT / mask type MT -- float, or the compact batch's bf16 / u8: the instantiation
    // is chosen with them, launch_flow_pair_forward)
    const void* image_ref;    // [B,3,H,W], H = o.crop_h, W = o.crop_w
    const void* image;
    const void* jitter_ref;   // [B,Cj,H,W]
    const void* jitter;
    int Cj;
    float* partial;           // [2B, T, 2]
    float thresh;
    // GRAD (mr_flow_pair_forward_grad_tiles): the thread holds everything the pair loss's backward needs -- taps, masks, the
    // epilogue's factors -- so it leaves d(sum of |residuals|) / d(rendered displacement) of its pixel, the "unit gradient"
    // (the backward multiplies by grad_loss / count, one scalar per image), and the tile's largest magnitude
    float* unit_grad;         // [2B, H, W, 2] (written under the covered tiles)
    unsigned* tile_max;       // [2B, T] float bits
    // REC (mr_pair_step_forward, round 6): the render left ONE 16-byte record per pixel {displacement x, y, alpha, mask} instead
    // of the planes of o.mask / o.flow / o.scale (unused then; o.occl may be NULL: nobody reads a pair step's occlusion maps)
    const float4* rec;        // [2B, is, is] image orientation: frame 1's B images, then frame 2's
};

template <bool GRAD, bool REC, PairCrit CRIT, typename IT = float, typename MT = float>
__device__ __forceinline__ void flow_pair_forward_tiles_body(const FlowPairFwdParams& q) {
    __shared__ float red[2][4][2];
    __shared__ unsigned redm[2][4];
    const OcclTilesParams& p = q.o;
    unsigned j;
    const ListSlice sl = list_slice(p.list.tlist->n_heavy, p.list.tlist->n_light, j);
    const int T = p.tiles_x * p.tiles_y, is = p.is, H = p.crop_h, W = p.crop_w;
    const int64_t hw = (int64_t)is * is, hw_img = (int64_t)H * W;
    unsigned round = 0;
    for (; j < sl.n_local; j += sl.stride) {
        const TileAt t = tile_at(p.list.ids[sl.slot(j, p.list.cap)].x, p.B, p.tiles_x, T, is, p.hit[0], p.hit[1]);
        // Round 6: the pixel's own values are requested TOGETHER with the tile's coverage word, not behind it (nine dependent
        // round trips per tile -- list header, entry, word, own values, byte at q, planes at q, byte at r, mask at r, taps --
        // were this kernel: six now, occl_from_own_together takes two more out).  What the planes hold under a row pair
        // without a covered pixel is discarded below; the addresses are inside the planes whatever the word says.
        const bool inside = t.x < is && t.ry < is;
        const int a = t.dir, o_ = 1 - t.dir;
        const float* ma = REC ? nullptr : p.mask[a] + (int64_t)t.b * hw;
        const float* fab = REC ? nullptr : p.flow[a] + (int64_t)t.b * p.fbstride;
        const float* sab = (!REC && p.scale[a]) ? p.scale[a] + (int64_t)t.b * hw : nullptr;
        const float4* rec_a = REC ? q.rec + ((int64_t)a * p.B + t.b) * hw : nullptr;
        const int64_t pix = (int64_t)t.y * is + t.x;
        const bool in_crop = inside && t.y < H && t.x < W;
        const int64_t pixc = (int64_t)t.y * W + t.x;
        // direction 0 = frame 1's grid: flow12 warps `image` towards image_ref, gated by jitter_ref; direction 1: the reverse
        const IT* src = static_cast<const IT*>(t.dir ? q.image_ref : q.image);
        const IT* tgt = static_cast<const IT*>(t.dir ? q.image : q.image_ref);
        const MT* jit = static_cast<const MT*>(t.dir ? q.jitter : q.jitter_ref);
        DirRaw2T<IT, MT> raw{};
        float ma_p = 0.0f, sc = 1.0f, f0 = 0.0f, f1 = 0.0f;
        if (in_crop) pair_load_own(tgt, jit, q.Cj, t.b, pixc, hw_img, raw);
        if (inside) {
            if constexpr (REC) {
                const float4 own = rec_a[pix];
                f0 = own.x; f1 = own.y; sc = own.w; ma_p = record_mask(own, a);
            } else {
                ma_p = ma[pix];
                if (sab) sc = sab[pix];
                f0 = fab[pix]; f1 = fab[hw + pix];
            }
        }
        pin(ma_p); pin(sc); pin(f0); pin(f1);  // (requested in front of the branch on the word, not sunk behind it)
        if (t.word == 0u) continue;  // (uniform)
        float sum = 0.0f, cnt = 0.0f;
        unsigned gmx = 0u;
        if (inside) {
            const uint8_t* ha = p.hit[a] + (int64_t)t.b * T * 4;
            const uint8_t* hb = p.hit[o_] + (int64_t)t.b * T * 4;
            // (the planes are defined wherever the row pair holds a covered pixel: elsewhere the values above are dropped)
            if (!t.row_covered) { ma_p = 0.0f; sc = 1.0f; f0 = 0.0f; f1 = 0.0f; }
            float o = 0.0f;
            if constexpr (REC) {
                if (t.row_covered && ma_p != 0.0f)
                    o = occl_from_own_records(ma_p, f0 * sc, f1 * sc, rec_a, q.rec + ((int64_t)o_ * p.B + t.b) * hw, a, is, is, t.x, t.y,
                                              p.dist_thresh, p.wthresh, ha, hb, p.tiles_x);
            } else {
                const float* mb = p.mask[o_] + (int64_t)t.b * hw;
                const float* fba = p.flow[o_] + (int64_t)t.b * p.fbstride;
                const float* sba = p.scale[o_] ? p.scale[o_] + (int64_t)t.b * hw : nullptr;
                if (t.row_covered && ma_p != 0.0f)
                    o = occl_from_own_together(ma_p, sab ? f0 * sc : f0, sab ? f1 * sc : f1, ma, mb, fba, sba, hw, is, is, t.x, t.y,
                                               p.dist_thresh, p.wthresh, ha, hb, p.tiles_x);
            }
            if (p.occl[a]) p.occl[a][(int64_t)t.b * hw + pix] = o;
            if (in_crop) {
                const float post = o != 0.0f ? ma_p * o : 0.0f;
                float2 r = make_float2(0.0f, 0.0f);
                if (post != 0.0f && sc != 0.0f) r = make_float2((f0 * sc) * post, (f1 * sc) * post);
                *reinterpret_cast<float2*>(p.out[a] + ((int64_t)t.b * hw_img + pixc) * 2) = r;
#pragma unroll
                for (int c = 0; c < 3; c++) pin(raw.tgt[c]);
                pin(raw.jd);
                float2 gq = make_float2(0.0f, 0.0f);
                if (r.x != 0.0f) {  // (a zero x component: invalid whatever the images hold, imgflowarp.py:93-100)
                    const DirTaps tp = pair_taps(r, t.x, t.y, H, W);
                    pair_load_taps(tp, src, jit, q.Cj, t.b, hw_img, raw);
                    pin(raw);
                    const DirRaw rr = unpack(raw, tp.a);
                    const DirOut e = pair_eval(tp, rr, H, W, q.thresh, false);
                    if (e.valid) {
#pragma unroll
                        for (int c = 0; c < 3; c++) sum += pair_term<CRIT>(e.s[c] - rr.tgt[c]);
                        cnt = 3.0f;
                    }
                    if (GRAD) {
                        // pair_consist_backward_tiles_kernel's gradient with coefficient 1, times the epilogue's factors as
                        // the raster backward applies them: (g * (mask_x * occl)) * mask_pre
                        const float2 gp = pair_grad<CRIT>(tp, rr, e, H, W, 1.0f);
                        gq = make_float2((gp.x * post) * sc, (gp.y * post) * sc);
                    }
                }
                if (GRAD) {
                    *reinterpret_cast<float2*>(q.unit_grad + ((int64_t)t.img * hw_img + pixc) * 2) = gq;
                    gmx = abs_bits_max(gq);
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { sum += __shfl_xor(sum, off); cnt += __shfl_xor(cnt, off); }
        if (GRAD) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) gmx = max(gmx, (unsigned)__shfl_xor((int)gmx, off));
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = round++ & 1u;  // (executed rounds only: see above)
        if (lane == 0) { red[slot][wave][0] = sum; red[slot][wave][1] = cnt; if (GRAD) redm[slot][wave] = gmx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float* out = q.partial + ((int64_t)t.img * T + t.tile) * 2;
            out[0] = red[slot][0][0] + red[slot][1][0] + red[slot][2][0] + red[slot][3][0];
            out[1] = red[slot][0][1] + red[slot][1][1] + red[slot][2][1] + red[slot][3][1];
            if (GRAD) q.tile_max[(int64_t)t.img * T + t.tile] = max(max(redm[slot][0], redm[slot][1]), max(redm[slot][2], redm[slot][3]));
        }
    }
}

// per-sample fixed-order reduction of the tile partials, counted only where the coverage words say a workgroup wrote one
// (the words and the partials of a tile are requested together: whatever an unwritten partial holds is discarded)
__global__ void __launch_bounds__(256) pair_consist_finalize_tiles_kernel(const float* __restrict__ partial,
                                                                          const uint32_t* __restrict__ hit12,
                                                                          const uint32_t* __restrict__ hit21, int B, int T,
                                                                          float* __restrict__ sums, float* __restrict__ loss_fwd,
                                                                          float* __restrict__ loss_bwd,
                                                                          const unsigned* __restrict__ tile_max,
                                                                          unsigned* __restrict__ image_max,
                                                                          float* __restrict__ loss_sum, ScatterWork work,
                                                                          unsigned* __restrict__ mean_ctr,
                                                                          float* __restrict__ mean_out, int mean_of,
                                                                          unsigned* __restrict__ list_reset) {
    // list_reset (mr_pair_step_forward): the three counters of the render's tile-list header.  This launch is the last of the
    // pair's forward side, and nothing behind the fused warp forward reads them: zeroed here, the NEXT pair step on this
    // scratch finds its list header clean (MR_PAIR_STEP_LIST_CLEAN) without a clearing launch in front of its binning pass.
    if (list_reset && blockIdx.x == 0 && threadIdx.x < 3) list_reset[threadIdx.x] = 0u;
    __shared__ float red[4][4];
    __shared__ unsigned redm[4][2];
    __shared__ int wcov[2][4][4];  // [direction][round of the chunk][wave]
    const int b = blockIdx.x;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned m12 = 0u, m21 = 0u;  // largest unit-gradient magnitude (float bits) of stack images b and B + b
    if (work.cov) {
        // ... and the ids of the covered tiles of stack images b and B + b, compacted (ascending) for the raster backward's
        // launch (ScatterWork, mr_common.hpp): this workgroup holds the coverage words of both anyway
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int base12 = 0, base21 = 0;
        // FIN_CH rounds of 256 tiles at a time: their words / partials are requested together and ONE barrier pair serves them
        // (round 6; a round per barrier pair before: 4 rounds of dependent loads and 8 barriers at 480 x 480, 7.0 us for the 8
        // workgroups of config 3).  The order of the sums (round by round per thread) and of the lists (ascending) is unchanged.
        constexpr int FIN_CH = 4;
        for (int t0 = 0; t0 < T; t0 += 256 * FIN_CH) {
            uint32_t h21[FIN_CH], h12[FIN_CH];
            float2 v1[FIN_CH], v2[FIN_CH];
            unsigned t21[FIN_CH], t12[FIN_CH];
#pragma unroll
            for (int u = 0; u < FIN_CH; u++) {
                h21[u] = 0u; h12[u] = 0u; v1[u] = make_float2(0.0f, 0.0f); v2[u] = v1[u]; t21[u] = 0u; t12[u] = 0u;
                if (t0 + u * 256 >= T) continue;  // (uniform: a 256-tile raster is ONE round, as before)
                const int t = t0 + u * 256 + (int)threadIdx.x;
                const int tc = t < T ? t : T - 1;
                h21[u] = hit21[(int64_t)b * T + tc]; h12[u] = hit12[(int64_t)b * T + tc];
                v1[u] = *reinterpret_cast<const float2*>(partial + ((int64_t)(B + b) * T + tc) * 2);
                v2[u] = *reinterpret_cast<const float2*>(partial + ((int64_t)b * T + tc) * 2);
                if (tile_max) { t21[u] = tile_max[(int64_t)(B + b) * T + tc]; t12[u] = tile_max[(int64_t)b * T + tc]; }
            }
            bool c21[FIN_CH], c12[FIN_CH];
            unsigned long long k12[FIN_CH], k21[FIN_CH];
#pragma unroll
            for (int u = 0; u < FIN_CH; u++) {
                c21[u] = false; c12[u] = false; k12[u] = 0ull; k21[u] = 0ull;
                if (t0 + u * 256 >= T) continue;
                const bool in = t0 + u * 256 + (int)threadIdx.x < T;
                c21[u] = in && h21[u] != 0u; c12[u] = in && h12[u] != 0u;
                if (c21[u]) { a[0] += v1[u].x; a[1] += v1[u].y; m21 = max(m21, t21[u]); }
                if (c12[u]) { a[2] += v2[u].x; a[3] += v2[u].y; m12 = max(m12, t12[u]); }
                k12[u] = __ballot(c12[u]); k21[u] = __ballot(c21[u]);
                if (lane == 0) { wcov[0][u][wave] = __popcll(k12[u]); wcov[1][u][wave] = __popcll(k21[u]); }
            }
            __syncthreads();
            const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
            for (int u = 0; u < FIN_CH; u++) {
                if (t0 + u * 256 >= T) continue;
                int o12 = base12, o21 = base21;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    o12 += w < wave ? wcov[0][u][w] : 0; o21 += w < wave ? wcov[1][u][w] : 0;
                    base12 += wcov[0][u][w]; base21 += wcov[1][u][w];
                }
                const int t = t0 + u * 256 + (int)threadIdx.x;
                if (c12[u]) work.cov[(int64_t)b * T + o12 + __popcll(k12[u] & below)] = (unsigned short)t;
                if (c21[u]) work.cov[(int64_t)(B + b) * T + o21 + __popcll(k21[u] & below)] = (unsigned short)t;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { work.n_cov[b] = base12; work.n_cov[B + b] = base21; }
    } else {
        for (int t = threadIdx.x; t < T; t += 256) {
            const uint32_t h21 = hit21[(int64_t)b * T + t], h12 = hit12[(int64_t)b * T + t];
            const float2 v1 = *reinterpret_cast<const float2*>(partial + ((int64_t)(B + b) * T + t) * 2);
            const float2 v2 = *reinterpret_cast<const float2*>(partial + ((int64_t)b * T + t) * 2);
            unsigned t21 = 0u, t12 = 0u;
            if (tile_max) { t21 = tile_max[(int64_t)(B + b) * T + t]; t12 = tile_max[(int64_t)b * T + t]; }
            if (h21 != 0u) { a[0] += v1.x; a[1] += v1.y; m21 = max(m21, t21); }
            if (h12 != 0u) { a[2] += v2.x; a[3] += v2.y; m12 = max(m12, t12); }
        }
    }
    if (image_max) {  // (uniform)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            m12 = max(m12, (unsigned)__shfl_xor((int)m12, off));
            m21 = max(m21, (unsigned)__shfl_xor((int)m21, off));
        }
        if ((threadIdx.x & 63) == 0) { redm[threadIdx.x >> 6][0] = m12; redm[threadIdx.x >> 6][1] = m21; }
    }
    block_sum4(a, red);  // (its barrier also publishes redm)
    if (threadIdx.x == 0 && image_max) {
        image_max[b] = max(max(redm[0][0], redm[1][0]), max(redm[2][0], redm[3][0]));
        image_max[B + b] = max(max(redm[0][1], redm[1][1]), max(redm[2][1], redm[3][1]));
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) sums[b * 4 + k] = a[k];
        const float n1 = (a[1] == 0.0f) ? 1.0f : a[1], n2 = (a[3] == 0.0f) ? 1.0f : a[3];
        if (loss_fwd) loss_fwd[b] = a[0] / n1;
        if (loss_bwd) loss_bwd[b] = a[2] / n2;
        if (loss_sum) loss_sum[b] = a[2] / n2 + a[0] / n1;  // pair_consist's warp_loss with use_backward (imgflowarp.py:104-113)
    }
    if (mean_out) {  // (uniform)
        // mr_pair_step_forward: the mean over the batch (warpbranch.py:87-88) by the workgroup that finishes LAST -- no launch of
        // its own (a 64-lane kernel costs 4.8 us on the timeline).  A sample's value crosses workgroups in an agent-scope atomic
        // store, the count in an agent-scope atomic add behind it (s_waitcnt in between: the store has completed), the last
        // arriver reads all B values with agent-scope atomic loads and sums them in a FIXED order (lane-strided partial sums in
        // index order, then a butterfly): the same bits whichever workgroup comes last.  The counter (a spare word of the render's
        // tile-list header, cleared with it) is re-zeroed for the next call.
        __shared__ int s_last_ws;
        if (threadIdx.x == 0) {
            const float n1 = (a[1] == 0.0f) ? 1.0f : a[1], n2 = (a[3] == 0.0f) ? 1.0f : a[3];
            const float mine = mean_of ? a[0] / n1 : a[2] / n2 + a[0] / n1;
            __hip_atomic_store(mean_out + 1 + b, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned old = __hip_atomic_fetch_add(mean_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last_ws = (old == (unsigned)B - 1u) ? 1 : 0;
            if (s_last_ws) __hip_atomic_store(mean_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (s_last_ws && threadIdx.x < 64) {
            float sacc = 0.0f;
            for (int i = threadIdx.x; i < B; i += 64) sacc += __hip_atomic_load(mean_out + 1 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) sacc += __shfl_xor(sacc, off);
            if (threadIdx.x == 0) mean_out[0] = sacc / (float)B;
        }
    }
}

template <PairCrit CRIT>
__device__ __forceinline__ void pair_consist_backward_tiles_body(const PairTilesParams& p) {
    unsigned j;
    const ListSlice sl = list_slice(p.list.tlist->n_heavy, p.list.tlist->n_light, j);
    const int T = p.tiles_x * p.tiles_y;
    const int64_t hw = (int64_t)p.H * p.W;
    for (; j < sl.n_local; j += sl.stride) {
        const TileAt t = tile_at(p.list.ids[sl.slot(j, p.list.cap)].x, p.B, p.tiles_x, T, p.is, p.hit[0], p.hit[1]);
        if (t.word == 0u) continue;
        unsigned u = 0u;
        if (t.x < p.W && t.y >= 0 && t.y < p.H) {
            const int64_t pix = (int64_t)t.y * p.W + t.x;
            float2 g = make_float2(0.0f, 0.0f);
            const float c = p.sums[t.b * 4 + (t.dir ? 1 : 3)];
            const float* gl = t.dir ? p.grad_loss_fwd : p.grad_loss_bwd;
            const float coef = gl ? pair_coef(gl[t.b], c) : 0.0f;
            if (t.row_covered && coef != 0.0f) {
                const float2 uv = pair_flow(p.flow[t.dir], t.b, t.x, t.y, p.H, p.W);
                if (uv.x != 0.0f) {  // the gradient of an invalid pixel is 0 (see the forward kernel)
                    const PairDir d = pair_dir(p, t.dir);
                    // (pair_pixel's sequence, and abs_bits_max below, spelled out: see pair_pixel)
                    const DirTaps tp = pair_taps(uv, t.x, t.y, p.H, p.W);
                    DirRaw2 q{};
                    pair_load(tp, d.src, d.tgt, d.jit, d.jit, p.Cj, false, t.b, pix, hw, q);
                    pin(q);
                    const DirRaw r = unpack(q, tp.a);
                    const DirOut e = pair_eval(tp, r, p.H, p.W, p.thresh, false);
                    g = pair_grad<CRIT>(tp, r, e, p.H, p.W, coef);
                }
            }
            *reinterpret_cast<float2*>(p.grad_flow[t.dir] + ((int64_t)t.b * hw + pix) * 2) = g;
            u = max(__float_as_uint(g.x) & 0x7fffffffu, __float_as_uint(g.y) & 0x7fffffffu);
        }
        // the largest |gradient| per image of the stack (see pair_consist_backward_kernel)
        if (p.grad_max && __ballot(u != 0u) != 0ull) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, off));
            if ((threadIdx.x & 63) == 0 && u > p.grad_max[t.img]) atomicMax(&p.grad_max[t.img], u);
        }
    }
}

// The kernels: one __global__ per criterion around each body (the l1 kernels keep their names -- profiles and the bench
// find them by name --, the l2 ones carry _l2); the host picks one per launch (MR_CRITERION_*).
__global__ void __launch_bounds__(256, 6) pair_consist_forward_tiles_kernel(PairTilesParams p) { pair_consist_forward_tiles_body<PairCrit::L1>(p); }
__global__ void __launch_bounds__(256, 6) pair_consist_forward_tiles_l2_kernel(PairTilesParams p) { pair_consist_forward_tiles_body<PairCrit::L2>(p); }
__global__ void __launch_bounds__(256) pair_consist_backward_tiles_kernel(PairTilesParams p) { pair_consist_backward_tiles_body<PairCrit::L1>(p); }
__global__ void __launch_bounds__(256) pair_consist_backward_tiles_l2_kernel(PairTilesParams p) { pair_consist_backward_tiles_body<PairCrit::L2>(p); }
template <bool GRAD, bool REC = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) flow_pair_forward_tiles_kernel(FlowPairFwdParams q) {
    flow_pair_forward_tiles_body<GRAD, REC, PairCrit::L1>(q);
}
template <bool GRAD, bool REC = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) flow_pair_forward_tiles_l2_kernel(FlowPairFwdParams q) {
    flow_pair_forward_tiles_body<GRAD, REC, PairCrit::L2>(q);
}
// ... on a compact image batch (MR_DTYPE_*): bf16 images with u8 or with fp32 jitter masks.  The same body; only its loads and
// the widening behind them know the element types.
template <bool GRAD, bool REC = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) flow_pair_forward_tiles_bf16u8_kernel(FlowPairFwdParams q) {
    flow_pair_forward_tiles_body<GRAD, REC, PairCrit::L1, bf16_t, uint8_t>(q);
}
template <bool GRAD, bool REC = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) flow_pair_forward_tiles_l2_bf16u8_kernel(FlowPairFwdParams q) {
    flow_pair_forward_tiles_body<GRAD, REC, PairCrit::L2, bf16_t, uint8_t>(q);
}
template <bool GRAD, bool REC = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) flow_pair_forward_tiles_bf16f32_kernel(FlowPairFwdParams q) {
    flow_pair_forward_tiles_body<GRAD, REC, PairCrit::L1, bf16_t, float>(q);
}
template <bool GRAD, bool REC = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) flow_pair_forward_tiles_l2_bf16f32_kernel(FlowPairFwdParams q) {
    flow_pair_forward_tiles_body<GRAD, REC, PairCrit::L2, bf16_t, float>(q);
}

}  // namespace mr

using namespace mr;

// ---- listed launches of the warp half (see the kernels) --------------------------------------------------------------
// (listed_grid, the workgroups of a launch over the render's tile list: launch_plan.hpp)

extern "C" int mr_occlusion_flow_tiles(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                       const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                       const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                       float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2, int batch_size,
                                       int image_size, int crop_height, int crop_width, float distance_thresh,
                                       float warp_thresh, const void* list_header, const void* list_entries,
                                       int64_t list_capacity, int64_t tile_bound, mr_stream_t stream) {
    if (!mask_flow1 || !mask_flow2 || !flow12 || !flow21 || !occl1 || !occl2 || !flow_out12 || !flow_out21 || !tile_hit1 ||
        !tile_hit2 || !list_header || !list_entries)
        return MR_ERR_BADARG;
    if (batch_size < 0 || image_size <= 0 || flow_bstride < 2LL * image_size * image_size) return MR_ERR_BADARG;
    if (crop_height <= 0 || crop_width <= 0 || crop_height > image_size || crop_width > image_size) return MR_ERR_BADARG;
    const int tiles_x = (image_size + 31) / 32, tiles_y = (image_size + 7) / 8;
    if (list_capacity != 2LL * batch_size * tiles_x * tiles_y || !grid_ok(list_capacity)) return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    OcclTilesParams p{{mask_flow1, mask_flow2}, {flow12, flow21}, {flow12_scale, flow21_scale}, {occl1, occl2},
                      {flow_out12, flow_out21}, {tile_hit1, tile_hit2}, flow_bstride, batch_size, image_size, crop_height,
                      crop_width, tiles_x, tiles_y, distance_thresh, warp_thresh,
                      {(const TileList*)list_header, (const uint4*)list_entries, (unsigned)list_capacity}};
    hipLaunchKernelGGL(occlusion_flow_tiles_kernel, dim3(listed_grid(tile_bound, list_capacity)), dim3(256), 0,
                       (hipStream_t)stream, p);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

// workspace of the listed pair loss, per tile of the 2B stacked images: {sum, count} of the pair loss | (mr_flow_pair_forward_grad_
// tiles) the largest unit gradient -- word arrays, packed.  Places them in `q` (nullable), returns the bytes.
static int64_t pair_tiles_work(void* ws, int batch_size, int hit_image_size, FlowPairFwdParams* q = nullptr) {
    const int64_t tiles = 2LL * batch_size * ((hit_image_size + 31) / 32) * ((hit_image_size + 7) / 8);
    Carve c;
    const int64_t partial = c.take(tiles * 2 * (int64_t)sizeof(float), 4), tile_max = c.take(tiles * (int64_t)sizeof(unsigned), 4);
    if (q) { q->partial = at_offset<float>(ws, partial); q->tile_max = at_offset<unsigned>(ws, tile_max); }
    return c.total();
}
extern "C" int64_t mr_pair_consist_tiles_workspace_bytes(int batch_size, int hit_image_size) {
    if (batch_size < 0 || hit_image_size <= 0) return MR_ERR_BADARG;
    return pair_tiles_work(nullptr, batch_size, hit_image_size);
}

extern "C" int64_t mr_flow_pair_scatter_work_bytes(int batch_size, int image_size) {
    if (batch_size < 0 || image_size <= 0) return MR_ERR_BADARG;
    return scatter_work_bytes(2 * batch_size, ((image_size + 31) / 32) * ((image_size + 7) / 8));
}

// the checks the listed pair-loss launches share; `p` (mr_pair_consist_*_tiles): gets the PairTilesParams fields they share
static int pair_tiles_args_ok(const float* flow12, const float* flow21, const float* image_ref, const float* image,
                              const float* jitter_ref, const float* jitter, int jitter_channels, int batch_size, int height,
                              int width, const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                              const void* list_header, const void* list_entries, int64_t list_capacity, float thresh = 0.0f,
                              PairTilesParams* p = nullptr) {
    if (!flow12 || !flow21 || !image_ref || !image || !jitter_ref || !jitter || !tile_hit12 || !tile_hit21 || !list_header ||
        !list_entries)
        return MR_ERR_BADARG;
    if (jitter_channels != 1 && jitter_channels != 3) return MR_ERR_BADARG;
    if (batch_size < 0 || height <= 0 || width <= 0 || hit_image_size < height || hit_image_size < width) return MR_ERR_BADARG;
    if (width < 2 || (int64_t)height * width > (1LL << 29)) return MR_ERR_BADARG;  // row-pair taps, 32-bit byte offsets
    const int64_t T = (int64_t)((hit_image_size + 31) / 32) * ((hit_image_size + 7) / 8);
    if (list_capacity != 2LL * batch_size * T || !grid_ok(list_capacity)) return MR_ERR_BADARG;
    if (!p) return MR_OK;
    p->flow[0] = flow12; p->flow[1] = flow21;
    p->image_ref = image_ref; p->image = image; p->jitter_ref = jitter_ref; p->jitter = jitter; p->Cj = jitter_channels;
    p->hit[0] = tile_hit12; p->hit[1] = tile_hit21;
    p->B = batch_size; p->H = height; p->W = width; p->is = hit_image_size;
    p->tiles_x = (hit_image_size + 31) / 32; p->tiles_y = (hit_image_size + 7) / 8;
    p->thresh = thresh;
    p->list = ListArgs{(const TileList*)list_header, (const uint4*)list_entries, (unsigned)list_capacity};
    return MR_OK;
}

extern "C" int mr_pair_consist_forward_tiles_crit(const float* flow12, const float* flow21, const float* image_ref,
                                                  const float* image, const float* jitter_ref, const float* jitter,
                                                  int jitter_channels, void* workspace, int64_t workspace_bytes, float* sums,
                                                  float* loss_fwd, float* loss_bwd, int batch_size, int height, int width,
                                                  float thresh, const uint8_t* tile_hit12, const uint8_t* tile_hit21,
                                                  int hit_image_size, const void* list_header, const void* list_entries,
                                                  int64_t list_capacity, int64_t tile_bound, mr_stream_t stream, int criterion) {
    if (!criterion_ok(criterion)) return MR_ERR_BADARG;
    PairTilesParams p{};
    const int rc = pair_tiles_args_ok(flow12, flow21, image_ref, image, jitter_ref, jitter, jitter_channels, batch_size, height, width,
                                      tile_hit12, tile_hit21, hit_image_size, list_header, list_entries, list_capacity, thresh, &p);
    if (rc != MR_OK) return rc;
    if (!workspace || !sums || workspace_bytes < mr_pair_consist_tiles_workspace_bytes(batch_size, hit_image_size))
        return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    p.partial = (float*)workspace;
    hipLaunchKernelGGL(criterion == MR_CRITERION_L2 ? pair_consist_forward_tiles_l2_kernel : pair_consist_forward_tiles_kernel,
                       dim3(listed_grid(tile_bound, list_capacity)), dim3(256), 0, (hipStream_t)stream, p);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(pair_consist_finalize_tiles_kernel, dim3(batch_size), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, reinterpret_cast<const uint32_t*>(tile_hit12),
                       reinterpret_cast<const uint32_t*>(tile_hit21), batch_size, p.tiles_x * p.tiles_y, sums, loss_fwd, loss_bwd,
                       (const unsigned*)nullptr, (unsigned*)nullptr, (float*)nullptr, ScatterWork{nullptr, nullptr},
                       (unsigned*)nullptr, (float*)nullptr, 0, (unsigned*)nullptr);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_pair_consist_forward_tiles(const float* flow12, const float* flow21, const float* image_ref,
                                             const float* image, const float* jitter_ref, const float* jitter,
                                             int jitter_channels, void* workspace, int64_t workspace_bytes, float* sums,
                                             float* loss_fwd, float* loss_bwd, int batch_size, int height, int width,
                                             float thresh, const uint8_t* tile_hit12, const uint8_t* tile_hit21,
                                             int hit_image_size, const void* list_header, const void* list_entries,
                                             int64_t list_capacity, int64_t tile_bound, mr_stream_t stream) {
    return mr_pair_consist_forward_tiles_crit(flow12, flow21, image_ref, image, jitter_ref, jitter, jitter_channels, workspace,
                                              workspace_bytes, sums, loss_fwd, loss_bwd, batch_size, height, width, thresh,
                                              tile_hit12, tile_hit21, hit_image_size, list_header, list_entries, list_capacity,
                                              tile_bound, stream, MR_CRITERION_L1);
}

extern "C" int mr_pair_consist_backward_tiles_crit(const float* flow12, const float* flow21, const float* image_ref,
                                                   const float* image, const float* jitter_ref, const float* jitter,
                                                   int jitter_channels, const float* sums, const float* grad_loss_fwd,
                                                   const float* grad_loss_bwd, float* grad_flow12, float* grad_flow21,
                                                   int batch_size, int height, int width, float thresh,
                                                   const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                                                   float* grad_max, const void* list_header, const void* list_entries,
                                                   int64_t list_capacity, int64_t tile_bound, mr_stream_t stream, int criterion) {
    if (!criterion_ok(criterion)) return MR_ERR_BADARG;
    PairTilesParams p{};
    const int rc = pair_tiles_args_ok(flow12, flow21, image_ref, image, jitter_ref, jitter, jitter_channels, batch_size, height, width,
                                      tile_hit12, tile_hit21, hit_image_size, list_header, list_entries, list_capacity, thresh, &p);
    if (rc != MR_OK) return rc;
    if (!sums || !grad_loss_fwd || !grad_flow12 || !grad_flow21) return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    p.sums = sums; p.grad_loss_fwd = grad_loss_fwd; p.grad_loss_bwd = grad_loss_bwd;
    p.grad_flow[0] = grad_flow12; p.grad_flow[1] = grad_flow21;
    p.grad_max = reinterpret_cast<unsigned*>(grad_max);
    hipLaunchKernelGGL(criterion == MR_CRITERION_L2 ? pair_consist_backward_tiles_l2_kernel : pair_consist_backward_tiles_kernel,
                       dim3(listed_grid(tile_bound, list_capacity)), dim3(256), 0, (hipStream_t)stream, p);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_pair_consist_backward_tiles(const float* flow12, const float* flow21, const float* image_ref,
                                              const float* image, const float* jitter_ref, const float* jitter,
                                              int jitter_channels, const float* sums, const float* grad_loss_fwd,
                                              const float* grad_loss_bwd, float* grad_flow12, float* grad_flow21,
                                              int batch_size, int height, int width, float thresh,
                                              const uint8_t* tile_hit12, const uint8_t* tile_hit21, int hit_image_size,
                                              float* grad_max, const void* list_header, const void* list_entries,
                                              int64_t list_capacity, int64_t tile_bound, mr_stream_t stream) {
    return mr_pair_consist_backward_tiles_crit(flow12, flow21, image_ref, image, jitter_ref, jitter, jitter_channels, sums,
                                               grad_loss_fwd, grad_loss_bwd, grad_flow12, grad_flow21, batch_size, height, width,
                                               thresh, tile_hit12, tile_hit21, hit_image_size, grad_max, list_header,
                                               list_entries, list_capacity, tile_bound, stream, MR_CRITERION_L1);
}


// the kernel of a plan: the batch's element types, the form (records / unit gradient / loss only) and the criterion
static void (*pair_forward_kernel(const PairFwdPlan& plan))(FlowPairFwdParams) {
    const bool l2 = plan.l2;
    switch (plan.types) {
    case PairFwdPlan::F32_F32:
        switch (plan.form) {
        case PairFwdPlan::RECORDS: return l2 ? flow_pair_forward_tiles_l2_kernel<true, true> : flow_pair_forward_tiles_kernel<true, true>;
        case PairFwdPlan::UNIT_GRAD: return l2 ? flow_pair_forward_tiles_l2_kernel<true> : flow_pair_forward_tiles_kernel<true>;
        case PairFwdPlan::LOSS_ONLY: return l2 ? flow_pair_forward_tiles_l2_kernel<false> : flow_pair_forward_tiles_kernel<false>;
        }
        break;
    case PairFwdPlan::BF16_U8:
        switch (plan.form) {
        case PairFwdPlan::RECORDS: return l2 ? flow_pair_forward_tiles_l2_bf16u8_kernel<true, true> : flow_pair_forward_tiles_bf16u8_kernel<true, true>;
        case PairFwdPlan::UNIT_GRAD: return l2 ? flow_pair_forward_tiles_l2_bf16u8_kernel<true> : flow_pair_forward_tiles_bf16u8_kernel<true>;
        case PairFwdPlan::LOSS_ONLY: return l2 ? flow_pair_forward_tiles_l2_bf16u8_kernel<false> : flow_pair_forward_tiles_bf16u8_kernel<false>;
        }
        break;
    case PairFwdPlan::BF16_F32:
        switch (plan.form) {
        case PairFwdPlan::RECORDS: return l2 ? flow_pair_forward_tiles_l2_bf16f32_kernel<true, true> : flow_pair_forward_tiles_bf16f32_kernel<true, true>;
        case PairFwdPlan::UNIT_GRAD: return l2 ? flow_pair_forward_tiles_l2_bf16f32_kernel<true> : flow_pair_forward_tiles_bf16f32_kernel<true>;
        case PairFwdPlan::LOSS_ONLY: return l2 ? flow_pair_forward_tiles_l2_bf16f32_kernel<false> : flow_pair_forward_tiles_bf16f32_kernel<false>;
        }
        break;
    }
    return nullptr;
}

int mr::launch_flow_pair_forward(const FlowPairFwdArgs& a, hipStream_t s) {
    const bool grad = a.unit_grad != nullptr;
    if (a.records ? (!grad || misaligned({a.records}, 15))
                  : (!a.mask_flow1 || !a.mask_flow2 || !a.flow12 || !a.flow21 || !a.occl1 || !a.occl2))
        return MR_ERR_BADARG;
    if (!a.flow_out12 || !a.flow_out21 || !criterion_ok(a.criterion)) return MR_ERR_BADARG;
    if (!image_dtype_ok(a.image_dtype) || !mask_dtype_ok(a.mask_dtype)) return MR_ERR_BADARG;
    if (a.image_dtype == MR_DTYPE_F32 && a.mask_dtype != MR_DTYPE_F32) return MR_ERR_NOTIMPL;  // (no fp32-image / u8-mask kernel)
    if (a.batch_size < 0 || a.image_size <= 0 || (!a.records && a.flow_bstride < 2LL * a.image_size * a.image_size)) return MR_ERR_BADARG;
    // (the shared checks look at the four batch pointers for NULL only)
    const float *im_ref = (const float*)a.image_ref, *im = (const float*)a.image, *jm_ref = (const float*)a.jitter_ref, *jm = (const float*)a.jitter;
    const int rc = pair_tiles_args_ok(a.flow_out12, a.flow_out21, im_ref, im, jm_ref, jm, a.jitter_channels,
                                      a.batch_size, a.height, a.width, a.tile_hit1, a.tile_hit2, a.image_size, a.list_header,
                                      a.list_entries, a.list_capacity);
    if (rc != MR_OK) return rc;
    FlowPairFwdParams q{};
    if (!a.workspace || !a.sums || a.workspace_bytes < pair_tiles_work(a.workspace, a.batch_size, a.image_size, &q)) return MR_ERR_BADARG;
    if (a.batch_size == 0) return MR_OK;
    const PairFwdPlan plan = plan_pair_forward(a.batch_size, a.image_size, a.records != nullptr, grad, a.criterion, a.image_dtype, a.mask_dtype,
                                               a.tile_bound, a.list_capacity);
    const TileList* header = (const TileList*)a.list_header;
    q.o = OcclTilesParams{{a.mask_flow1, a.mask_flow2}, {a.flow12, a.flow21}, {a.flow12_scale, a.flow21_scale}, {a.occl1, a.occl2},
                          {a.flow_out12, a.flow_out21}, {a.tile_hit1, a.tile_hit2}, a.flow_bstride, a.batch_size, a.image_size,
                          a.height, a.width, plan.tiles_x, plan.tiles_y, a.distance_thresh, a.warp_thresh,
                          {header, (const uint4*)a.list_entries, (unsigned)a.list_capacity}};
    q.image_ref = a.image_ref; q.image = a.image; q.jitter_ref = a.jitter_ref; q.jitter = a.jitter; q.Cj = a.jitter_channels;
    q.thresh = a.pair_thresh;
    q.unit_grad = a.unit_grad;
    q.rec = (const float4*)a.records;
    hipLaunchKernelGGL(pair_forward_kernel(plan), dim3(plan.wgs), dim3(256), 0, s, q);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(pair_consist_finalize_tiles_kernel, dim3(plan.finalize_wgs), dim3(256), 0, s, (const float*)a.workspace,
                       reinterpret_cast<const uint32_t*>(a.tile_hit1), reinterpret_cast<const uint32_t*>(a.tile_hit2), a.batch_size,
                       plan.tiles_x * plan.tiles_y, a.sums, a.loss_fwd, a.loss_bwd, grad ? (const unsigned*)q.tile_max : (const unsigned*)nullptr,
                       grad ? reinterpret_cast<unsigned*>(a.unit_grad_max) : (unsigned*)nullptr, a.loss_sum,
                       scatter_work_at(grad ? a.scatter_work : nullptr, 2 * a.batch_size),
                       // (the arrival counter of the batch mean: a spare word of the list header the caller cleared with it)
                       a.mean_out ? const_cast<unsigned*>(&header->pad[0]) : (unsigned*)nullptr, a.mean_out, a.mean_of,
                       a.reset_list ? const_cast<unsigned*>(&header->n_heavy) : (unsigned*)nullptr);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_flow_pair_forward_grad_tiles_typed(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                                    const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                                    const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                                    float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2,
                                                    const void* image_ref, const void* image, const void* jitter_ref,
                                                    const void* jitter, int jitter_channels, void* workspace,
                                                    int64_t workspace_bytes, float* sums, float* loss_fwd, float* loss_bwd,
                                                    int batch_size, int image_size, int height, int width, float distance_thresh,
                                                    float warp_thresh, float pair_thresh, const void* list_header,
                                                    const void* list_entries, int64_t list_capacity, int64_t tile_bound,
                                                    float* unit_grad, float* unit_grad_max, float* loss_sum,
                                                    void* scatter_work, mr_stream_t stream, int criterion, int image_dtype, int mask_dtype) {
    if (!unit_grad || !unit_grad_max) return MR_ERR_BADARG;
    FlowPairFwdArgs a{};
    a.mask_flow1 = mask_flow1; a.mask_flow2 = mask_flow2; a.flow12 = flow12; a.flow21 = flow21; a.flow_bstride = flow_bstride;
    a.flow12_scale = flow12_scale; a.flow21_scale = flow21_scale;
    a.occl1 = occl1; a.occl2 = occl2; a.flow_out12 = flow_out12; a.flow_out21 = flow_out21;
    a.tile_hit1 = tile_hit1; a.tile_hit2 = tile_hit2;
    a.image_ref = image_ref; a.image = image; a.jitter_ref = jitter_ref; a.jitter = jitter; a.jitter_channels = jitter_channels;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    a.sums = sums; a.loss_fwd = loss_fwd; a.loss_bwd = loss_bwd;
    a.batch_size = batch_size; a.image_size = image_size; a.height = height; a.width = width;
    a.distance_thresh = distance_thresh; a.warp_thresh = warp_thresh; a.pair_thresh = pair_thresh;
    a.list_header = list_header; a.list_entries = list_entries; a.list_capacity = list_capacity; a.tile_bound = tile_bound;
    a.unit_grad = unit_grad; a.unit_grad_max = unit_grad_max; a.loss_sum = loss_sum; a.scatter_work = scatter_work;
    a.criterion = criterion; a.image_dtype = image_dtype; a.mask_dtype = mask_dtype;
    return launch_flow_pair_forward(a, (hipStream_t)stream);
}

extern "C" int mr_flow_pair_forward_grad_tiles_crit(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                                    const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                                    const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                                    float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2,
                                                    const float* image_ref, const float* image, const float* jitter_ref,
                                                    const float* jitter, int jitter_channels, void* workspace,
                                                    int64_t workspace_bytes, float* sums, float* loss_fwd, float* loss_bwd,
                                                    int batch_size, int image_size, int height, int width, float distance_thresh,
                                                    float warp_thresh, float pair_thresh, const void* list_header,
                                                    const void* list_entries, int64_t list_capacity, int64_t tile_bound,
                                                    float* unit_grad, float* unit_grad_max, float* loss_sum,
                                                    void* scatter_work, mr_stream_t stream, int criterion) {
    return mr_flow_pair_forward_grad_tiles_typed(mask_flow1, mask_flow2, flow12, flow21, flow_bstride, flow12_scale,
        flow21_scale, occl1, occl2, flow_out12, flow_out21, tile_hit1, tile_hit2, image_ref, image, jitter_ref, jitter,
        jitter_channels, workspace, workspace_bytes, sums, loss_fwd, loss_bwd, batch_size, image_size, height, width,
        distance_thresh, warp_thresh, pair_thresh, list_header, list_entries, list_capacity, tile_bound, unit_grad,
        unit_grad_max, loss_sum, scatter_work, stream, criterion, MR_DTYPE_F32, MR_DTYPE_F32);
}

extern "C" int mr_flow_pair_forward_grad_tiles(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                               const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                               const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                               float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2,
                                               const float* image_ref, const float* image, const float* jitter_ref,
                                               const float* jitter, int jitter_channels, void* workspace,
                                               int64_t workspace_bytes, float* sums, float* loss_fwd, float* loss_bwd,
                                               int batch_size, int image_size, int height, int width, float distance_thresh,
                                               float warp_thresh, float pair_thresh, const void* list_header,
                                               const void* list_entries, int64_t list_capacity, int64_t tile_bound,
                                               float* unit_grad, float* unit_grad_max, float* loss_sum,
                                               void* scatter_work, mr_stream_t stream) {
    return mr_flow_pair_forward_grad_tiles_crit(mask_flow1, mask_flow2, flow12, flow21, flow_bstride, flow12_scale, flow21_scale,
                                                occl1, occl2, flow_out12, flow_out21, tile_hit1, tile_hit2, image_ref, image,
                                                jitter_ref, jitter, jitter_channels, workspace, workspace_bytes, sums, loss_fwd,
                                                loss_bwd, batch_size, image_size, height, width, distance_thresh, warp_thresh,
                                                pair_thresh, list_header, list_entries, list_capacity, tile_bound, unit_grad,
                                                unit_grad_max, loss_sum, scatter_work, stream, MR_CRITERION_L1);
}

extern "C" int mr_flow_pair_forward_tiles_typed(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                               const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                               const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                               float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2,
                                               const void* image_ref, const void* image, const void* jitter_ref,
                                               const void* jitter, int jitter_channels, void* workspace, int64_t workspace_bytes,
                                               float* sums, float* loss_fwd, float* loss_bwd, int batch_size, int image_size,
                                               int height, int width, float distance_thresh, float warp_thresh, float pair_thresh,
                                               const void* list_header, const void* list_entries, int64_t list_capacity,
                                               int64_t tile_bound, mr_stream_t stream, int criterion, int image_dtype, int mask_dtype) {
    FlowPairFwdArgs a{};
    a.mask_flow1 = mask_flow1; a.mask_flow2 = mask_flow2; a.flow12 = flow12; a.flow21 = flow21; a.flow_bstride = flow_bstride;
    a.flow12_scale = flow12_scale; a.flow21_scale = flow21_scale;
    a.occl1 = occl1; a.occl2 = occl2; a.flow_out12 = flow_out12; a.flow_out21 = flow_out21;
    a.tile_hit1 = tile_hit1; a.tile_hit2 = tile_hit2;
    a.image_ref = image_ref; a.image = image; a.jitter_ref = jitter_ref; a.jitter = jitter; a.jitter_channels = jitter_channels;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    a.sums = sums; a.loss_fwd = loss_fwd; a.loss_bwd = loss_bwd;
    a.batch_size = batch_size; a.image_size = image_size; a.height = height; a.width = width;
    a.distance_thresh = distance_thresh; a.warp_thresh = warp_thresh; a.pair_thresh = pair_thresh;
    a.list_header = list_header; a.list_entries = list_entries; a.list_capacity = list_capacity; a.tile_bound = tile_bound;
    a.criterion = criterion; a.image_dtype = image_dtype; a.mask_dtype = mask_dtype;
    return launch_flow_pair_forward(a, (hipStream_t)stream);
}

extern "C" int mr_flow_pair_forward_tiles_crit(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                               const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                               const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                               float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2,
                                               const float* image_ref, const float* image, const float* jitter_ref,
                                               const float* jitter, int jitter_channels, void* workspace, int64_t workspace_bytes,
                                               float* sums, float* loss_fwd, float* loss_bwd, int batch_size, int image_size,
                                               int height, int width, float distance_thresh, float warp_thresh, float pair_thresh,
                                               const void* list_header, const void* list_entries, int64_t list_capacity,
                                               int64_t tile_bound, mr_stream_t stream, int criterion) {
    return mr_flow_pair_forward_tiles_typed(mask_flow1, mask_flow2, flow12, flow21, flow_bstride, flow12_scale, flow21_scale,
        occl1, occl2, flow_out12, flow_out21, tile_hit1, tile_hit2, image_ref, image, jitter_ref, jitter, jitter_channels,
        workspace, workspace_bytes, sums, loss_fwd, loss_bwd, batch_size, image_size, height, width, distance_thresh,
        warp_thresh, pair_thresh, list_header, list_entries, list_capacity, tile_bound, stream, criterion, MR_DTYPE_F32,
        MR_DTYPE_F32);
}

extern "C" int mr_flow_pair_forward_tiles(const float* mask_flow1, const float* mask_flow2, const float* flow12,
                                          const float* flow21, int64_t flow_bstride, const float* flow12_scale,
                                          const float* flow21_scale, float* occl1, float* occl2, float* flow_out12,
                                          float* flow_out21, const uint8_t* tile_hit1, const uint8_t* tile_hit2,
                                          const float* image_ref, const float* image, const float* jitter_ref,
                                          const float* jitter, int jitter_channels, void* workspace, int64_t workspace_bytes,
                                          float* sums, float* loss_fwd, float* loss_bwd, int batch_size, int image_size,
                                          int height, int width, float distance_thresh, float warp_thresh, float pair_thresh,
                                          const void* list_header, const void* list_entries, int64_t list_capacity,
                                          int64_t tile_bound, mr_stream_t stream) {
    return mr_flow_pair_forward_tiles_crit(mask_flow1, mask_flow2, flow12, flow21, flow_bstride, flow12_scale, flow21_scale, occl1,
                                           occl2, flow_out12, flow_out21, tile_hit1, tile_hit2, image_ref, image, jitter_ref, jitter,
                                           jitter_channels, workspace, workspace_bytes, sums, loss_fwd, loss_bwd, batch_size,
                                           image_size, height, width, distance_thresh, warp_thresh, pair_thresh, list_header,
                                           list_entries, list_capacity, tile_bound, stream, MR_CRITERION_L1);
}
