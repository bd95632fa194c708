// raster_bwd_vc.hip -- backward of the rasteriser for gfx950 (MI355X), the training path: the gradient w.r.t. the
// per-vertex colours of the vertex-colour mode, and the tile scatter that folds the flow epilogue's adjoint and the pair
// loss's backward into it.  The upstream-compatible backward (E / F gather, kernel D) is in raster_bwd.hip; neither
// file includes the other (the map accessors both use are in mr_common.hpp).
//
// Kernels, in file order:
//   * gather_vc_kernel -- the face-parallel gather of raster_bwd.hip's gather_kernel for the vertex-colour mode, with an
//     LDS fragment ring (probe, compact the won pixels, shade with full lanes); kept as the fallback for meshes whose
//     colour table does not fit LDS.
//   * scatter_vc_kernel<STORED> -- E for the vertex-colour mode: PIXEL-parallel, block-private [V,3] table in LDS in
//     64-bit fixed point, optionally on the forward's stored weight / depth maps (see the comment at the kernel).
//   * scatter_tiles_kernel<FLOWGRAD, REC> -- the same table, the pixels walked over the forward's covered tiles
//     (scatter_tiles_body and its named phases); FLOWGRAD: the gradient is the flow's, taken through the epilogue's adjoint.
//   * pair_scatter_tiles_kernel, pair_scatter_tiles_l2_kernel -- ... with the pair loss's backward folded into pass 1.
//   * unit_scatter_listing_kernel, unit_scatter_tiles_kernel -- ... with the pair loss's unit gradient already formed by
//     the forward launch; the second hands its workgroups out over the forward's covered-tile lists (what the step launches).
//
// Entry points: mr_render_vc_backward, mr_render_flow_backward, mr_flow_pair_backward_tiles_crit,
// mr_flow_pair_backward_tiles, mr_flow_pair_backward_unit_tiles, and mr::launch_unit_scatter_tiles for pair_step.hip.
#include "mr_common.hpp"
#include "pair_launch.hpp"
#include "warp_device.hpp"
#include <algorithm>
#include <type_traits>

namespace mr {

// GLPF lanes per face: lane `sub` walks bbox rows sub, sub + lanes, ...; the partial sums are combined with shuffles inside
// the lane group (fixed order: deterministic).  Faces whose bbox exceeds GATHER_BIG pixels are walked by the whole wave
// instead.  (GLPF: launch_plan.hpp)
constexpr int GATHER_BIG = 128;          // vertex-colour gather: bbox area above which the whole wave probes
// (256 until round 5: the 114 faces of the bench scene with boxes of 256-500 pixels then took the whole-wave path ONE BEHIND THE
// OTHER inside the wave that holds them -- consecutive wrist faces -- while as ordinary lane groups they advance side by side: E
// alone 93.7 -> 90.4 us at 256 x 256, 263 -> 230 at 640 x 640; 8192: no further gain at 256, slower at 640)

// ---------------------------------------------------------------------------------------
// E for the vertex-colour mode: gradient w.r.t. the per-vertex colours, fill-back by index
// ---------------------------------------------------------------------------------------
struct GatherVCParams {
    const float* verts;     // [B,V,3] projected
    const int32_t* fidx;    // [B,F0,3]
    const int32_t* fim;     // raster orientation, values in [0, 2 F0)
    const float* grad_rgb;  // image orientation
    float* grad_vcolors;    // [B,V,3], pre-zeroed, accumulated with fp32 atomics
    int B, V, F0, fill_back, is;
    float eps;
    int texel;  // texel layout code of the vertex-colour texture (mr_common.hpp: texel_vertex)
};

// contribution of one won pixel to the colours of the face's three vertices (its own order)
__device__ __forceinline__ void gather_vc_pixel(const GatherVCParams& p, const Face& f, int b, int xi, int yi,
                                                float (*acc)[3]) {
    float w[3], zp, tif[3], g[3];
    bary(f, xi, yi, zp, w);
    tex_coords(w, zp, f.v, 2, p.eps, tif);
#pragma unroll
    for (int c = 0; c < 3; c++) g[c] = p.grad_rgb[idx3<true>(b, yi, xi, c, p.is)];
    // taps pn = 1, 2, 4 are the texels holding the colours of vertices 0, 1, 2
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int pn = 1 << k;
        float wg = 1.0f;
#pragma unroll
        for (int j = 0; j < 3; j++) wg *= ((pn >> j) & 1) ? (tif[j] - 0.0f) : (1.0f - (tif[j] - 0.0f));
#pragma unroll
        for (int c = 0; c < 3; c++) acc[k][c] += wg * g[c];
    }
}

// GLPF lanes per REAL face, 16 faces per wave.  Pass 0 handles every face's visible orientation
// (normally exactly one of the two fill-back orientations is front-facing), pass 1 the second
// orientation of zero-area faces.  Per pass, three lock-step stages mirror the forward kernel:
//   P1 one lane of the quad: orientation's vertices + inverse into an LDS face cache;
//   P2 the quad probes the face's bbox in face_index_map (lane k: rows k, k+4, ...; 8 probes in
//      flight per iteration) and appends the pixels the face WON as fragments (slot, dx, dy) to
//      an LDS ring (ballot compaction); faces with a large bbox are probed by the whole wave;
//   P3 lane per fragment, 64 at a time: barycentrics, sampling weights, gradient of the three
//      vertex colours, accumulated per face in LDS (ds_add_f32).
// The per-face sums go to grad_vcolors with 9 global fp32 atomics per live face.
constexpr int GV_SLOTS = MR_WAVE / GLPF;  // faces per wave
constexpr int GV_FCS = 23;    // dwords per face-cache slot (odd stride)
constexpr int GV_FQ = 1024;   // fragment ring capacity (>= 63 + 8 * 64, power of 2)

template <int DUMMY>
__global__ void __launch_bounds__(256) gather_vc_kernel(GatherVCParams p) {
    __shared__ float fcache[4][GV_SLOTS * GV_FCS];
    __shared__ float facc[4][GV_SLOTS * 9];
    __shared__ unsigned fragq[4][GV_FQ];

    const int64_t total = (int64_t)p.B * p.F0;
    const int64_t gid = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    const int64_t i = gid / GLPF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % GLPF, slot_own = lane / GLPF;
    const bool valid = i < total;
    const int b = valid ? (int)(i / p.F0) : 0;
    const int f0 = valid ? (int)(i % p.F0) : 0;
    const int is = p.is;
    float* fc = fcache[wave];
    float* fa = facc[wave];
    unsigned* fq = fragq[wave];
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    int vid[3] = {0, 0, 0};
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = __builtin_nanf("");
    if (valid) {
        const int32_t* ix = p.fidx + i * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            vid[k] = ix[k];
            const float* g = p.verts + ((int64_t)b * p.V + vid[k]) * 3;
            v[3 * k] = g[0]; v[3 * k + 1] = g[1]; v[3 * k + 2] = g[2];
        }
    }
    float acc[3][3];  // [real vertex][channel]
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[k][c] = 0.0f;
    const int32_t* fim_b = p.fim + (int64_t)b * is * is;
    // P3: one lane per fragment
    int qhead = 0, qn = 0;
    auto shade = [&](int n) {
        if (lane < n) {
            const unsigned fr = fq[(qhead + lane) & (GV_FQ - 1)];
            const int slot = (int)(fr >> 26);
            const float* c = fc + slot * GV_FCS;
            Face f;
#pragma unroll
            for (int k = 0; k < 9; k++) f.inv[k] = c[9 + k];
            f.v[2] = c[2]; f.v[5] = c[5]; f.v[8] = c[8];
            const int xi = __float_as_int(c[18]) + (int)(fr & 0x1fffu), yi = __float_as_int(c[19]) + (int)((fr >> 13) & 0x1fffu);
            const int bb = __float_as_int(c[20]);
            float w[3], zp, tif[3], g[3];
            bary(f, xi, yi, zp, w);
            tex_coords(w, zp, f.v, 2, p.eps, tif);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) g[ch] = p.grad_rgb[idx3<true>(bb, yi, xi, ch, is)];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int pn = 1 << k;
                float wg = 1.0f;
#pragma unroll
                for (int j = 0; j < 3; j++) wg *= ((pn >> j) & 1) ? (tif[j] - 0.0f) : (1.0f - (tif[j] - 0.0f));
#pragma unroll
                for (int ch = 0; ch < 3; ch++) atomicAdd(&fa[slot * 9 + k * 3 + ch], wg * g[ch]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    // which orientations can be visible (normally exactly one: the front-facing one)
    bool live[2];
    {
        float r[9];
#pragma unroll
        for (int k = 0; k < 3; k++) { r[k] = v[6 + k]; r[3 + k] = v[3 + k]; r[6 + k] = v[k]; }
        const FaceBox ba = face_box(v, is), bb2 = face_box(r, is);
        live[0] = valid && ba.x0 <= ba.x1;
        live[1] = valid && p.fill_back && bb2.x0 <= bb2.x1;
    }
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        // pass 0: every face's first live orientation; pass 1: the second one where BOTH are live
        // (zero-area faces only)
        const int o = pass == 0 ? (live[0] ? 0 : 1) : 1;
        const bool mine = pass == 0 ? (live[0] || live[1]) : (live[0] && live[1]);
        Face f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int s = o ? 2 - k : k;
            f.v[3 * k] = v[3 * s]; f.v[3 * k + 1] = v[3 * s + 1]; f.v[3 * k + 2] = v[3 * s + 2];
        }
        FaceBox bx = face_box(f.v, is);
        if (!mine) { bx.x0 = 1; bx.x1 = 0; bx.y0 = 1; bx.y1 = 0; }
        const bool nonempty = mine && bx.x0 <= bx.x1;
        const int bw = bx.x1 - bx.x0 + 1, bh = bx.y1 - bx.y0 + 1;
        const bool big = nonempty && bw * bh > GATHER_BIG;
        const int fn = o ? f0 + p.F0 : f0;
        if (__ballot(nonempty) == 0ull) continue;  // wave-uniform

        // P1: park the orientation's face in the cache, clear its accumulators
        if (sub == 0) {
            float* c = fc + slot_own * GV_FCS;
            if (nonempty) {
                face_inverse(f.v, f.inv, is);
#pragma unroll
                for (int k = 0; k < 9; k++) { c[k] = f.v[k]; c[9 + k] = f.inv[k]; }
                c[18] = __int_as_float((int)bx.x0); c[19] = __int_as_float((int)bx.y0); c[20] = __int_as_float(b);
            }
#pragma unroll
            for (int k = 0; k < 9; k++) fa[slot_own * 9 + k] = 0.0f;
        }
        __builtin_amdgcn_wave_barrier();

        // P2 (large faces): the whole wave probes the bbox, lane per column, rows in groups of 8;
        // won pixels join the same fragment ring
        unsigned long long m_big = __ballot(big && sub == 0);
        while (m_big) {
            const int src = __ffsll((long long)m_big) - 1;
            m_big &= m_big - 1;
            const int x0 = __shfl((int)bx.x0, src), y0 = __shfl((int)bx.y0, src);
            const int w_ = __shfl(bw, src), h_ = __shfl(bh, src);
            const int ff = __shfl(fn, src);
            const int32_t* fim_s = p.fim + (int64_t)__shfl(b, src) * is * is;  // the wave may straddle two images
            for (int cx0 = 0; cx0 < w_; cx0 += MR_WAVE) {
                const int cx = cx0 + lane;
                const bool col = cx < w_;
                for (int r = 0; r < h_; r += 8) {
                    int hit[8];
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        hit[u] = col ? fim_s[min(y0 + r + u, y0 + h_ - 1) * is + x0 + cx] : -2;
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const bool won = col && r + u < h_ && hit[u] == ff;
                        const unsigned long long m = __ballot(won);
                        if (won)
                            fq[(qhead + qn + __popcll(m & lt_mask)) & (GV_FQ - 1)] =
                                ((unsigned)(src / GLPF) << 26) | ((unsigned)(r + u) << 13) | (unsigned)cx;
                        qn += __popcll(m);
                    }
                    __builtin_amdgcn_wave_barrier();
                    while (qn >= MR_WAVE) {
                        shade(MR_WAVE);
                        qhead = (qhead + MR_WAVE) & (GV_FQ - 1);
                        qn -= MR_WAVE;
                    }
                }
            }
        }

        // P2: GLPF lanes per face (rows sub, sub + GLPF, ...), 8 probes per iteration, lock step
        bool act = nonempty && !big;
        int px = bx.x0, py = bx.y0 + sub;
        act = act && py <= bx.y1;
        while (__ballot(act) != 0ull) {
            int hit[8];
#pragma unroll
            for (int u = 0; u < 8; u++) hit[u] = act ? fim_b[py * is + min(px + u, (int)bx.x1)] : -2;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const bool won = act && px + u <= bx.x1 && hit[u] == fn;
                const unsigned long long m = __ballot(won);
                if (won)
                    fq[(qhead + qn + __popcll(m & lt_mask)) & (GV_FQ - 1)] =
                        ((unsigned)slot_own << 26) | ((unsigned)(py - bx.y0) << 13) | (unsigned)(px + u - bx.x0);
                qn += __popcll(m);
            }
            if (act) {
                px += 8;
                if (px > bx.x1) { px = bx.x0; py += GLPF; }
                act = py <= bx.y1;
            }
            __builtin_amdgcn_wave_barrier();
            while (qn >= MR_WAVE) {
                shade(MR_WAVE);
                qhead = (qhead + MR_WAVE) & (GV_FQ - 1);
                qn -= MR_WAVE;
            }
        }
        if (qn > 0) {
            shade(qn);
            qhead = (qhead + qn) & (GV_FQ - 1);
            qn = 0;
        }
        // collect this orientation's sums, mapped back to the real vertex order
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                // tap k of this orientation holds the colour of its vertex texel_vertex(k), i.e. of the REAL face's
                // vertex at position (o ? 2 - that : that)
                const int tv = texel_vertex(p.texel, k, o != 0);
                const int real = o ? 2 - tv : tv;
                const float add = fa[slot_own * 9 + k * 3 + c];
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q][c] += (q == real) ? add : 0.0f;
            }
        __builtin_amdgcn_wave_barrier();
    }
    if (valid && sub == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float* o = p.grad_vcolors + ((int64_t)b * p.V + vid[k]) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (acc[k][c] != 0.0f) atomicAdd(&o[c], acc[k][c]);
        }
    }
}

// ---------------------------------------------------------------------------------------
// E for the vertex-colour mode, pixel-parallel: the default when the per-image colour table fits LDS
// ---------------------------------------------------------------------------------------
// One block owns a SV_W x SV_H pixel region of one image, one lane per pixel (SV_RPW rows per
// wave).  face_index_map is read once, coalesced (a wave = one 64-pixel row segment, 256 B);
// regions without geometry leave after that single load.  A covered pixel needs its rgb gradient,
// the winner's index triple and -- STORED: the barycentric weights and depth the forward pass
// wrote for this very pixel plus the three vertex depths; else: the three projected vertices, from
// which inverse, weights and depth are recomputed with the forward's arithmetic.  All of these
// loads are issued before the first use (two round trips after face_index_map).  The 9 products
// (sampling weight x gradient channel) are added into a block-private [V,3] table in LDS, which is
// flushed with one global fp32 atomic per touched (vertex, channel): a few thousand per image
// instead of 9 per visible face, and no probing of face bounding boxes at all.
//
// The LDS table is 64-bit FIXED POINT, not fp32: ds_add_f32 is several times slower than the
// integer LDS atomics on gfx950 (measured: the 9 float adds per pixel cost more than everything
// else in this kernel together).  Every product w * g is bounded by the largest |g| of the region
// (the sampling weights are in [0,1]), so with that maximum < 2^e the products are scaled by
// 2^(SV_FIX_BITS - e), truncated to int64 and summed exactly; <= 3 * SV_W * SV_H terms of
// magnitude < 2^SV_FIX_BITS cannot overflow.  The absolute error per term is 2^-50 of the region's
// largest gradient -- far below fp32 rounding of the sum -- and the block's sums do not depend on
// the order of the additions.  Regions whose gradient holds an Inf / NaN take a plain fp32
// global-atomic path so that non-finite values propagate as they do in the gather kernel.
// (SV_WAVES waves per block, SV_RPW rows per wave of a SV_W x SV_H region, SV_MAX_TABLE_BYTES of colour table: launch_plan.hpp)
static_assert(WAVE == MR_WAVE, "the plans count lanes in waves of MR_WAVE");
constexpr int SV_FIX_BITS = 50;
static_assert(3LL * SV_W * SV_H < (1LL << (63 - SV_FIX_BITS)), "fixed-point sums must not overflow");

struct ScatterVCParams {
    GatherVCParams g;
    const float* weight;  // STORED: [B,is,is,3] raster orientation
    const float* depth;   // STORED: [B,is,is] image orientation
    int rx_n, ry_n;
};

template <bool STORED>
__global__ void __launch_bounds__(SV_WAVES * MR_WAVE) scatter_vc_kernel(ScatterVCParams sp) {
    extern __shared__ long long vtab[];  // [V * 3] rounded up to an even count
    __shared__ unsigned wmax[SV_WAVES];

    const GatherVCParams& p = sp.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned blk = xcd_remap(blockIdx.x, gridDim.x);
    const int rx = (int)(blk % (unsigned)sp.rx_n), ry = (int)((blk / (unsigned)sp.rx_n) % (unsigned)sp.ry_n);
    const int b = (int)(blk / (unsigned)(sp.rx_n * sp.ry_n));
    const int is = p.is;
    const int32_t* fim_b = p.fim + (int64_t)b * is * is;
    const int xi = rx * SV_W + lane, yi0 = ry * SV_H + wave * SV_RPW;

    int fnv[SV_RPW];
#pragma unroll
    for (int r = 0; r < SV_RPW; r++) fnv[r] = (xi < is && yi0 + r < is) ? fim_b[(yi0 + r) * is + xi] : -1;
    bool cov = false;
#pragma unroll
    for (int r = 0; r < SV_RPW; r++) cov = cov || fnv[r] >= 0;
    if (!__syncthreads_or(cov)) return;  // block-uniform

    const float* verts_b = p.verts + (int64_t)b * p.V * 3;
    const int32_t* fidx_b = p.fidx + (int64_t)b * p.F0 * 3;
    float g[SV_RPW][3], w[SV_RPW][3], zp[SV_RPW];
    int vid[SV_RPW][3];
    bool rev_r[SV_RPW];
#pragma unroll
    for (int r = 0; r < SV_RPW; r++) {
        const bool won = fnv[r] >= 0;
        const bool o = fnv[r] >= p.F0;  // reversed copy of face fn - F0
        rev_r[r] = o;
        const int32_t* ix = fidx_b + (int64_t)(won ? (o ? fnv[r] - p.F0 : fnv[r]) : 0) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) vid[r][k] = won ? ix[o ? 2 - k : k] : 0;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) g[r][ch] = won ? p.grad_rgb[idx3<true>(b, yi0 + r, xi, ch, is)] : 0.0f;
        if (STORED) {
            const float* wq = sp.weight + idx1<false>(b, yi0 + r, xi, is) * 3;
#pragma unroll
            for (int k = 0; k < 3; k++) w[r][k] = won ? wq[k] : 0.0f;
            zp[r] = won ? sp.depth[idx1<true>(b, yi0 + r, xi, is)] : 1.0f;
        }
    }
    Face f[SV_RPW];  // STORED: only the three depths v[2], v[5], v[8] are loaded
#pragma unroll
    for (int r = 0; r < SV_RPW; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float* q = verts_b + (int64_t)vid[r][k] * 3;
            const bool won = fnv[r] >= 0;
            if (!STORED) { f[r].v[3 * k] = won ? q[0] : 0.0f; f[r].v[3 * k + 1] = won ? q[1] : 0.0f; }
            f[r].v[3 * k + 2] = won ? q[2] : 1.0f;
        }

    // largest |gradient| over the region's covered pixels, as float bits
    unsigned mx = 0u;
#pragma unroll
    for (int r = 0; r < SV_RPW; r++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) mx = max(mx, __float_as_uint(g[r][ch]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
    if (lane == 0) wmax[wave] = mx;
    const int n2 = (p.V * 3 + 1) >> 1;
    for (int k = threadIdx.x; k < n2; k += blockDim.x) reinterpret_cast<int4*>(vtab)[k] = make_int4(0, 0, 0, 0);
    __syncthreads();  // table zeroed, maxima visible

    unsigned bm = 0u;
#pragma unroll
    for (int k = 0; k < SV_WAVES; k++) bm = max(bm, wmax[k]);
    if (bm == 0u) return;                   // every gradient of the region is +-0: nothing to add
    const bool finite = bm < 0x7f800000u;   // else: fp32 global atomics, Inf / NaN propagate
    const int shift = SV_FIX_BITS - ((int)(bm >> 23) - 126);  // largest |g| < 2^((bm >> 23) - 126)
    float* out = p.grad_vcolors + (int64_t)b * p.V * 3;

#pragma unroll
    for (int r = 0; r < SV_RPW; r++) {
        if (fnv[r] >= 0) {
            float tif[3];
            if (!STORED) {
                face_inverse(f[r].v, f[r].inv, is);
                bary(f[r], xi, yi0 + r, zp[r], w[r]);
            }
            tex_coords(w[r], zp[r], f[r].v, 2, p.eps, tif);
            // taps pn = 1, 2, 4 are the texels holding the colours of vertices 0, 1, 2
            float val[9];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int pn = 1 << k;
                float wg = 1.0f;
#pragma unroll
                for (int j = 0; j < 3; j++) wg *= ((pn >> j) & 1) ? (tif[j] - 0.0f) : (1.0f - (tif[j] - 0.0f));
#pragma unroll
                for (int ch = 0; ch < 3; ch++) val[k * 3 + ch] = wg * g[r][ch];
            }
            // Neighbouring lanes hold pixels of the same face or of faces sharing a vertex, and an
            // LDS atomic serialises lanes that hit one address.  Lane l therefore issues its nine
            // adds in the order (l % 9), (l % 9) + 1, ... so that the lanes of a run work on
            // different (vertex, channel) cells in any one instruction.
            const int rot = lane % 9;
#pragma unroll
            for (int bit = 1; bit < 16; bit <<= 1) {
                float t[9];
#pragma unroll
                for (int k = 0; k < 9; k++) t[k] = val[(k + bit) % 9];
                const bool on = (rot & bit) != 0;
#pragma unroll
                for (int k = 0; k < 9; k++) val[k] = on ? t[k] : val[k];
            }
#pragma unroll
            for (int j = 0; j < 9; j++) {
                int sl = j + rot;
                sl = sl >= 9 ? sl - 9 : sl;
                const int k = (sl >= 3) + (sl >= 6), ch = sl - 3 * k;
                const int cell = sel3(vid[r][0], vid[r][1], vid[r][2], texel_vertex(p.texel, k, rev_r[r])) * 3 + ch;
                if (finite) {
                    const long long q = (long long)ldexp((double)val[j], shift);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&vtab[cell]), (unsigned long long)q);
                } else if (val[j] != 0.0f) {
                    atomicAdd(&out[cell], val[j]);
                }
            }
        }
    }
    if (!finite) return;  // block-uniform
    __syncthreads();
    for (int k = threadIdx.x; k < p.V * 3; k += blockDim.x) {
        const long long t = vtab[k];
        if (t != 0) {
            const float v = (float)ldexp((double)t, -shift);
            if (v != 0.0f) atomicAdd(&out[k], v);
        }
    }
}

// ---------------------------------------------------------------------------------------
// E for the flow-mode render (mr_render_flow_backward): tile-persistent scatter
// ---------------------------------------------------------------------------------------
// The forward pass left one byte per (32x8 tile, row pair) saying whether anything is covered there (~17 % of the
// tiles of a hand + object frame).  ST_G workgroups of 4 waves share an image; every wave walks its own interleaved
// subset of the image's tiles, skips the empty ones on that byte (one scalar load -- the region kernel above
// dispatches 16 waves per 64x32 region only to find 70 % of them empty: 16 us of its 50 are wave dispatch), and
// handles a covered tile alone: lane = 4 consecutive pixels of a row, so that one wave-wide 16-byte load fetches a
// whole tile of a plane and a lane has four independent gather chains (face -> vertex ids -> vertex depths) in
// flight.  The [V,3] fixed-point table in LDS is zeroed and flushed once per WORKGROUP (a quarter image), not once
// per region; its scale comes from a first pass over the gradient of the workgroup's covered tiles.
// FLOWGRAD: the incoming gradient is the FLOW-space gradient [B,H,W,2] plus the masks of opticalflow.py:146-154 --
// the adjoint of crop / permute / mask products is applied on the fly with the arithmetic of
// flow_finalize_backward_kernel ((g * (m_x * occl)) * m_pre; third colour plane: zero), so that the [B,3,is,is]
// colour-space gradient is never materialised.
// Launch shape.  The [V, channels] fixed-point table is what limits residency (42.7 KB for a hand + object mesh with
// three channels: 3 workgroups per compute unit, 768 for 2048 launched, i.e. three rounds of ~9 us each -- workgroup
// timeline, profiles/r05_bwd_timeline_before.txt).  The flow-space gradient has two channels (the third colour plane's gradient is
// identically zero): its table is a third smaller; and eight workgroups of EIGHT waves per image instead of sixteen of
// four keep the 64 waves per image while halving the per-image fixed work (covered-tile list, table zeroing, flush):
// 4 x 8 waves fit a compute unit, so all 1024 workgroups of a 128-image launch are resident at once.
// (ST_G workgroups per image or more, ST_WAVES waves each, ST_TW x ST_TH tiles, ST_MAX_TILES of them per image: launch_plan.hpp)
static_assert(ST_TW == TILE_W && ST_TH == TILE_H, "the scatter walks the forward's tiles");

struct ScatterTilesParams {
    GatherVCParams g;
    const float* weight;        // [B,is,is,3] raster orientation, valid at covered pixels
    const float* depth;         // [B,is,is] image orientation, valid at covered pixels
    const uint32_t* tile_hit;   // [B, tiles] one byte per wave (row pair) of the forward's tile kernel; nullable
    const int32_t* vid_map;     // nullable: [B,is,is,3] vertex ids of the winner, written by mr_render_flow_forward; then
                                // `weight` holds the three sampling weights of the colour taps (not barycentrics)
    // FLOWGRAD
    const float* grad_flow;     // [B,H,W,2]
    const float* m_pre;         // [B,is,is] image orientation
    const float* m_x_lo;        // images [0, split)
    const float* m_x_hi;        // images [split, B)
    const float* occl;
    int split, H, W;
    int tiles_x, tiles_y;
    int groups;  // workgroups per image
    const float* grad_bound;  // nullable (FLOWGRAD): [B] upper bounds of |grad_flow| per image
    // PAIR (mr_flow_pair_backward_tiles): the pair loss's backward folded in -- pass 1 computes the flow gradient of the
    // workgroup's tiles itself (it used to be a kernel of its own + 8 B per pixel written and read back)
    float* stash;             // [B,H,W,2] scratch: the masked flow-space gradient, pass 1 -> pass 2 of the same workgroup
    const float* flow;        // [B,H,W,2] the stacked final flows (images [0, split): flow12, [split, B): flow21)
    const float* image_ref;   // [split,3,H,W]
    const float* image;
    const float* jitter_ref;  // [split,Cj,H,W]
    const float* jitter;
    int Cj;
    const float* sums;        // [split,4] of the pair loss's forward
    const float* gl_fwd;      // [split] incoming gradients of loss_fwd / loss_bwd (gl_bwd nullable)
    const float* gl_bwd;
    // UNIT (mr_pair_step_backward): two more incoming gradients, added to both directions' coefficients: of loss_bwd + loss_fwd
    // [split] and of the mean over the batch [1] (a sample's share = *gl_mean / mean_div), each nullable
    const float* gl_sum;
    const float* gl_mean;
    float mean_div;
    int mean_of;              // 1: the mean is over loss_fwd only -- no share for the other direction
    float pair_thresh;
    // UNIT (mr_flow_pair_backward_unit_tiles): the forward (mr_flow_pair_forward_grad_tiles) left the pair loss's gradient for
    // a coefficient of 1, masks applied; this launch multiplies by grad_loss / count of the image -- no taps, no pass 1
    const float* unit_grad;   // [B,H,W,2]
    const float* unit_max;    // [B] largest |unit gradient| per image (an upper bound is enough)
    // WORK (round 5): the images' covered-tile lists the forward's finalize launch left (mr_common.hpp, ScatterWork)
    ScatterWork work;
};

template <bool FLOWGRAD, bool PAIR = false, bool UNIT = false>
__device__ __forceinline__ void st_load_grad(const ScatterTilesParams& sp, int b, int yi, int x, float (*g)[3], float ucoef = 0.0f) {
    const GatherVCParams& p = sp.g;
    const int is = p.is;
    const int yimg = is - 1 - yi;
    if (PAIR || UNIT) {  // pass 1 of this workgroup (UNIT: the forward launch) left the gradient, masks applied
        const float* st = UNIT ? sp.unit_grad : sp.stash;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float2 gf = make_float2(0.0f, 0.0f);
            if (yimg < sp.H && x + j < sp.W) gf = *reinterpret_cast<const float2*>(st + (((int64_t)b * sp.H + yimg) * sp.W + x + j) * 2);
            g[j][0] = UNIT ? gf.x * ucoef : gf.x; g[j][1] = UNIT ? gf.y * ucoef : gf.y; g[j][2] = 0.0f;
        }
    } else if (!FLOWGRAD) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float4 v = *reinterpret_cast<const float4*>(p.grad_rgb + (((int64_t)b * 3 + ch) * is + yimg) * is + x);
            g[0][ch] = v.x; g[1][ch] = v.y; g[2][ch] = v.z; g[3][ch] = v.w;
        }
    } else {
        const int64_t o = ((int64_t)b * is + yimg) * is + x;
        const float* mx = b < sp.split ? sp.m_x_lo + o : sp.m_x_hi + (o - (int64_t)sp.split * is * is);
        const float4 a4 = *reinterpret_cast<const float4*>(sp.m_pre + o);
        const float4 x4 = *reinterpret_cast<const float4*>(mx);
        const float4 o4 = *reinterpret_cast<const float4*>(sp.occl + o);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        const float post[4] = {x4.x * o4.x, x4.y * o4.y, x4.z * o4.z, x4.w * o4.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float2 gf = make_float2(0.0f, 0.0f);
            const bool in = yimg < sp.H && x + j < sp.W;
            if (in) gf = *reinterpret_cast<const float2*>(sp.grad_flow + (((int64_t)b * sp.H + yimg) * sp.W + x + j) * 2);
            g[j][0] = in ? (gf.x * post[j]) * a[j] : 0.0f;
            g[j][1] = in ? (gf.y * post[j]) * a[j] : 0.0f;
            g[j][2] = 0.0f;
        }
    }
}

// ---- phases of scatter_tiles_body, each over what it is handed.  The stretches that stay in the body are there because every
// function form tried for them changed the compiled kernels (profiles/scatter_phases_isa.txt).

// flush: the table's sums, back to floats and added to the image's gradient
template <int NCH>
__device__ __forceinline__ void st_flush(const long long* vtab, int V, int shift, float* out) {
    for (int k = threadIdx.x; k < V * NCH; k += blockDim.x) {
        const long long tsum = (long long)((unsigned long long)vtab[k] << (64 - ST_SUM_BITS - 1)) >> (64 - ST_SUM_BITS - 1);
        if (tsum != 0) {
            const float v = (float)ldexp((double)tsum, -shift);
            if (v != 0.0f) atomicAdd(&out[(k / NCH) * 3 + k % NCH], v);
        }
    }
}

// bound, PAIR (pass 1): the pair loss's backward for the tiles of workgroup `part` of the G that share the image's list
// (pair_consist_backward_tiles_kernel's arithmetic, one pixel per thread, two tiles at a time), times the epilogue masks as
// st_load_grad forms them, into the stash; the largest |gradient| comes out on the way, in mx.  A final flow with a zero x
// component (everything the masks or the occlusion check removed) has a zero gradient: no taps.
template <bool WORK, PairCrit CRIT, typename TileAt>
__device__ __forceinline__ void st_pair_pass1(const ScatterTilesParams& sp, int b, int part, int G, int n_hits, int T, TileAt tile_at, unsigned& mx) {
    const int is = sp.g.is;
    const int n_mine = st_tiles_walked(n_hits, part, G);
    const int half = threadIdx.x >> 8, tid = threadIdx.x & 255;
    const int dir = b >= sp.split ? 1 : 0, pb = b - dir * sp.split;
    const float cnt = sp.sums[pb * 4 + (dir ? 1 : 3)];
    const float* gl = dir ? sp.gl_fwd : sp.gl_bwd;
    const float coef = gl ? pair_coef(gl[pb], cnt) : 0.0f;
    const float* src = dir ? sp.image_ref : sp.image;
    const float* tgt = dir ? sp.image : sp.image_ref;
    const float* jit = dir ? sp.jitter : sp.jitter_ref;
    const int64_t hw_img = (int64_t)sp.H * sp.W;
    for (int m = half; m < n_mine; m += 2) {
        const int t = tile_at(part * ST_WAVES + (m % ST_WAVES) + (m / ST_WAVES) * G * ST_WAVES);
        const int x = (t % sp.tiles_x) * ST_TW + (tid & 31), ry = (t / sp.tiles_x) * ST_TH + (tid >> 5);
        const int y = is - 1 - ry;
        if (x >= sp.W || ry >= is || y >= sp.H) continue;
        const int64_t pixc = (int64_t)y * sp.W + x;
        float2 gq = make_float2(0.0f, 0.0f);
        // the coverage word, the flow and the epilogue masks of the pixel are requested TOGETHER (all inside their
        // allocations; what an uncovered row pair holds there is never used): the taps are the only dependent trip
        const uint32_t word = sp.tile_hit[(int64_t)b * T + t];
        const int64_t o = ((int64_t)b * is + y) * is + x;
        float2 uv = *reinterpret_cast<const float2*>(sp.flow + ((int64_t)b * hw_img + pixc) * 2);
        float a = sp.m_pre[o];
        float mxo = (b < sp.split ? sp.m_x_lo[o] : sp.m_x_hi[o - (int64_t)sp.split * is * is]), oc = sp.occl[o];
        pin(uv.x); pin(uv.y); pin(a); pin(mxo); pin(oc);
        if (coef != 0.0f && ((word >> (8 * ((ry & 7) >> 1))) & 0xffu) != 0u) {
            if (uv.x != 0.0f) {
                const float post = mxo * oc;
                // (pair_pixel's sequence, spelled out: see pair_pixel)
                const DirTaps tp = pair_taps(uv, x, y, sp.H, sp.W);
                DirRaw2 q{};
                pair_load(tp, src, tgt, jit, jit, sp.Cj, false, pb, pixc, hw_img, q);
                pin(q);
                const DirRaw r = unpack(q, tp.a);
                const DirOut e = pair_eval(tp, r, sp.H, sp.W, sp.pair_thresh, false);
                const float2 gp = pair_grad<CRIT>(tp, r, e, sp.H, sp.W, coef);
                gq = make_float2((gp.x * post) * a, (gp.y * post) * a);
            }
        }
        *reinterpret_cast<float2*>(sp.stash + ((int64_t)b * hw_img + pixc) * 2) = gq;
        mx = max(mx, abs_bits_max(gq));
    }
}

// coefficient, UNIT: the image's scalars -- count, sum of the incoming loss gradients, bound of the unit gradient ...
struct StUnit {
    float cnt, gl, max;
};
__device__ __forceinline__ void st_unit_scalars(const ScatterTilesParams& sp, int b, StUnit& u) {
    const int dir = b >= sp.split ? 1 : 0, pb = b - dir * sp.split;
    const float* gl = dir ? sp.gl_fwd : sp.gl_bwd;
    u.cnt = sp.sums[pb * 4 + (dir ? 1 : 3)];
    u.gl = gl ? gl[pb] : 0.0f;
    if (sp.gl_sum) u.gl += sp.gl_sum[pb];
    if (sp.gl_mean && (dir || !sp.mean_of)) u.gl += sp.gl_mean[0] / sp.mean_div;
    u.max = sp.unit_max[b];
}
// ... and its coefficient (pair_consist_backward_tiles_kernel's): every gradient of the image is unit * coefficient, and
// |unit| <= unit_max rounds to at most fl(unit_max * |coefficient|) (rounding is monotone): the bound of the fixed point, left in
// mx as float bits.  A zero coefficient leaves the image without a gradient whatever the unit gradient holds: mx stays 0.
__device__ __forceinline__ float st_unit_coef(const ScatterTilesParams& sp, int b, const StUnit& u, unsigned& mx) {
    const float* gl = (b >= sp.split) ? sp.gl_fwd : sp.gl_bwd;
    const float ucoef = (gl || sp.gl_sum || sp.gl_mean) ? pair_coef(u.gl, u.cnt) : 0.0f;
    if (ucoef != 0.0f) mx = __float_as_uint(u.max * ucoef) & 0x7fffffffu;
    return ucoef;
}

// accumulate (pass 2), a lane's loads for its four pixels of a covered tile: gradient, weights, and the forward's records (REC)
// or the depth
template <bool FLOWGRAD, bool REC, bool PAIR, bool UNIT>
__device__ __forceinline__ void st_tile_loads(const ScatterTilesParams& sp, int b, int yi, int x, float ucoef, float (&g)[4][3], float (&w)[4][3],
                                              int (&vid)[4][3], float (&zp)[4]) {
    const int is = sp.g.is;
    st_load_grad<FLOWGRAD, PAIR, UNIT>(sp, b, yi, x, g, ucoef);
    const float4* wq = reinterpret_cast<const float4*>(sp.weight + (((int64_t)b * is + yi) * is + x) * 3);
    const float4 w0 = wq[0], w1 = wq[1], w2 = wq[2];
    w[0][0] = w0.x; w[0][1] = w0.y; w[0][2] = w0.z; w[1][0] = w0.w; w[1][1] = w1.x; w[1][2] = w1.y;
    w[2][0] = w1.z; w[2][1] = w1.w; w[2][2] = w2.x; w[3][0] = w2.y; w[3][1] = w2.z; w[3][2] = w2.w;
    if (REC) {
        // per-pixel records of the forward: the winner's vertex ids next to its sampling weights -- every load
        // of the pixel group is in flight at once, no index -> vertex chain
        const int4* vq = reinterpret_cast<const int4*>(sp.vid_map + (((int64_t)b * is + yi) * is + x) * 3);
        const int4 v0 = vq[0], v1 = vq[1], v2 = vq[2];
        vid[0][0] = v0.x; vid[0][1] = v0.y; vid[0][2] = v0.z; vid[1][0] = v0.w; vid[1][1] = v1.x; vid[1][2] = v1.y;
        vid[2][0] = v1.z; vid[2][1] = v1.w; vid[2][2] = v2.x; vid[3][0] = v2.y; vid[3][1] = v2.z; vid[3][2] = v2.w;
    } else {
        const float4 d4 = *reinterpret_cast<const float4*>(sp.depth + ((int64_t)b * is + (is - 1 - yi)) * is + x);
        zp[0] = d4.x; zp[1] = d4.y; zp[2] = d4.z; zp[3] = d4.w;
    }
}

// The body of the eight scatter kernels, phase by phase: 1. the workgroup's image and its list of covered tiles (WORK: a share
// of the forward's list; else the listing into LDS), 2. the image's coefficient (UNIT), 3. the bound of the gradients (pass 1:
// the caller's, the coefficient's, or a pass over the tiles -- PAIR: which forms the gradients on the way), 4. the scale of the
// fixed point, 5. the additions into the table (pass 2), 6. the flush.  Every barrier and fence is in this function.
template <bool FLOWGRAD, bool REC, bool PAIR, bool UNIT = false, bool WORK = false, PairCrit CRIT = PairCrit::L1>
__device__ __forceinline__ void scatter_tiles_body(const ScatterTilesParams& sp) {
    extern __shared__ long long vtab[];  // [V * NCH] rounded up to an even count
    constexpr int NCH = FLOWGRAD ? 2 : 3;  // (the flow-space gradient has no third channel)
    __shared__ unsigned wmax[ST_WAVES];
    __shared__ unsigned short hits[WORK ? 1 : ST_MAX_TILES];  // the image's covered tiles, ascending
    const GatherVCParams& p = sp.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int G = sp.groups;
    // PAIR: an image's workgroups on the XCD whose L2 holds what the forward launches just wrote for it (their tile lists are
    // image-major and every XCD takes a contiguous eighth: images [x B / 8, (x + 1) B / 8) on XCD x, more or less)
    const unsigned lidx = (PAIR || FLOWGRAD) ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    int b = (int)(lidx / (unsigned)G), part = (int)(lidx % (unsigned)G);
    const int is = p.is;
    const int T = sp.tiles_x * sp.tiles_y;
    int n_hits = 0;
    // 1. WORK: the table is zeroed FIRST (it needs nothing but V), so that the barrier behind it can wait where the first LDS
    // atomic is about to be issued -- behind the tile's loads instead of in front of them
    if constexpr (WORK)
        for (int k = threadIdx.x; k < (p.V * NCH + 1) >> 1; k += blockDim.x) reinterpret_cast<int4*>(vtab)[k] = make_int4(0, 0, 0, 0);
    const unsigned short* cov_b = nullptr;  // WORK: this workgroup's share of the forward's list of the image's covered tiles
    int t_first = 0;
    auto tile_at = [&](int h) -> int { return WORK ? (h == wave ? t_first : (int)cov_b[h]) : (int)hits[h]; };
    if constexpr (WORK) {
        // The launch's workgroups are handed out over the images IN PROPORTION TO THEIR COVERED TILES.  With a
        // fixed number per image the images that cover more than G x ST_WAVES tiles need a second round of their waves while
        // the waves of the others idle: on the bench scene (45 covered tiles per image on average, 8 x 8 waves) a third of the
        // workgroups ran two rounds and the launch ended at 18.8 us with the average workgroup done at 12.5
        // (profiles/r05_bwd_timeline_before.txt).  Every wave derives the split from the per-image counts the forward's
        // finalize launch left: q = tiles per workgroup (at least one per wave) such that sum ceil(n_b / q) fits the grid,
        // image b gets ceil(n_b / q) workgroups sharing its n_b tiles evenly, and the workgroups in use are spread over the
        // logical index range so that every XCD gets the same share.  No listing pass, no LDS list.  (The scalar arithmetic of
        // the split is launch_plan.hpp's, st_parts ... st_share, shared with the host test; the sums over the images are wave
        // scans and stay here.)
        const int B2 = p.B, grid = (int)gridDim.x;
        const int* ncov = sp.work.n_cov;
        // (every quantity below is the same in all lanes: readlane keeps it in scalar registers; the scans are DPP row shifts,
        // six vector instructions each, no LDS crossbar)
        // First try: one tile per wave (q = ST_WAVES) -- it fits whenever the scene leaves the grid some room, and then ONE pass
        // over the counts gives everything; else st_second_q and a second pass.  The counts of the first 4 x 64 images
        // are requested TOGETHER and stay in registers for all passes (one round trip; further images: read again, from L1).
        constexpr int NC = 4;
        int nreg[NC];
#pragma unroll
        for (int i = 0; i < NC; i++) nreg[i] = i * MR_WAVE + lane < B2 ? ncov[i * MR_WAVE + lane] : 0;
        int q = ST_WAVES, used = 0, N = 0;
#pragma unroll
        for (int i = 0; i < NC; i++) {
            if (i * MR_WAVE >= B2) break;
            N += __builtin_amdgcn_readlane(wave_incl_sum(nreg[i], lane), MR_WAVE - 1);
            used += __builtin_amdgcn_readlane(wave_incl_sum(st_parts(nreg[i], ST_WAVES), lane), MR_WAVE - 1);
        }
        for (int c = NC * MR_WAVE; c < B2; c += MR_WAVE) {
            const int n = c + lane < B2 ? ncov[c + lane] : 0;
            N += __builtin_amdgcn_readlane(wave_incl_sum(n, lane), MR_WAVE - 1);
            used += __builtin_amdgcn_readlane(wave_incl_sum(st_parts(n, ST_WAVES), lane), MR_WAVE - 1);
        }
        if (used > grid) {
            q = st_second_q(N, grid, B2);
            used = 0;
#pragma unroll
            for (int i = 0; i < NC; i++) {
                if (i * MR_WAVE >= B2) break;
                used += __builtin_amdgcn_readlane(wave_incl_sum(st_parts(nreg[i], q), lane), MR_WAVE - 1);
            }
            for (int c = NC * MR_WAVE; c < B2; c += MR_WAVE) {
                const int n = c + lane < B2 ? ncov[c + lane] : 0;
                used += __builtin_amdgcn_readlane(wave_incl_sum(st_parts(n, q), lane), MR_WAVE - 1);
            }
            used = st_used(used, grid);
        }
        // logical index -> slot k of the `used` workgroups with work, every XCD the same share of them (st_slot)
        int k;
        if ((grid & 7) == 0) {
            const StSlot sl = st_slot((int)lidx, grid, used);
            if (sl.j >= sl.n) return;
            k = sl.k0 + sl.j;
        } else {
            if ((int)lidx >= used) return;
            k = (int)lidx;
        }
        int base = 0, nb = 0, pb = 1;
        b = -1;
        for (int c = 0; c < B2 && b < 0; c += MR_WAVE) {
            const int ci = c / MR_WAVE;
            const int n = ci == 0 ? nreg[0] : ci == 1 ? nreg[1] : ci == 2 ? nreg[2] : ci == 3 ? nreg[3]
                                                                                         : (c + lane < B2 ? ncov[c + lane] : 0);
            const int parts = st_parts(n, q);
            const int incl = wave_incl_sum(parts, lane);
            const unsigned long long mine = __ballot(k >= base + incl - parts && k < base + incl);
            if (mine != 0ull) {
                const int src = __ffsll((long long)mine) - 1;
                b = c + src;
                part = k - (base + __builtin_amdgcn_readlane(incl - parts, src));
                nb = __builtin_amdgcn_readlane(n, src);
                pb = __builtin_amdgcn_readlane(parts, src);
            }
            base += __builtin_amdgcn_readlane(incl, MR_WAVE - 1);
        }
        if (b < 0) return;  // (cannot happen: k < used)
        // this workgroup's share of the image's list: tiles [first, first + n_hits); its waves take them round-robin
        const StShare sh = st_share(nb, pb, part);
        n_hits = sh.n;
        cov_b = sp.work.cov + (int64_t)b * T + sh.first;
        part = 0; G = 1;
        // (the wave's first tile id is requested now: its round trip runs beside the image's scalars and the table zeroing)
        t_first = wave < n_hits ? (int)cov_b[wave] : 0;
    }
    const int r = lane >> 3, x4 = (lane & 7) * 4;  // the lane's pixel quad inside a tile
    const int32_t* fim_b = p.fim + (int64_t)b * is * is;
    const float* verts_b = p.verts + (int64_t)b * p.V * 3;
    const int32_t* fidx_b = p.fidx + (int64_t)b * p.F0 * 3;

    // 2. UNIT: the image's scalars are requested NOW, in front of the coverage words, not behind the list they do not depend
    // on (one cold round trip less on the workgroup's chain); the coefficient is formed from them in 3.
    StUnit unit{1.0f, 0.0f, 0.0f};
    if constexpr (UNIT) st_unit_scalars(sp, b, unit);
    // 1. !WORK: the list of covered tiles (block-wide compaction of the coverage bytes); the waves that share an image then
    // take them round-robin: every wave gets its share whatever part of the screen the mesh sits in.  (All coverage words
    // requested up front and compacted behind one barrier -- eight predicated rounds unrolled -- measured SLOWER than
    // this loop at 1024 tiles per image: 1.98 against 1.54 us.)
    __shared__ int wcnt[ST_WAVES];
    if constexpr (!WORK)
    for (int t0 = 0; t0 < T; t0 += blockDim.x) {
        const int t = t0 + threadIdx.x;
        const bool hit = t < T && (sp.tile_hit ? sp.tile_hit[(int64_t)b * T + t] != 0u : true);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int base = n_hits;
        for (int w = 0; w < wave; w++) base += wcnt[w];
        if (hit) hits[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)t;
        for (int w = 0; w < ST_WAVES; w++) n_hits += wcnt[w];
        __syncthreads();
    }

    if (part * ST_WAVES >= n_hits) return;  // fewer covered tiles than waves before this workgroup: nothing to do
    if constexpr (!WORK) {
        const int n2 = (p.V * NCH + 1) >> 1;
        for (int k = threadIdx.x; k < n2; k += blockDim.x) reinterpret_cast<int4*>(vtab)[k] = make_int4(0, 0, 0, 0);
    }

    // 3. pass 1: largest |gradient| over the workgroup's covered tiles, as float bits -- or the caller's bound for the image
    unsigned mx = 0u;
    const bool bounded = PAIR || UNIT || (FLOWGRAD && sp.grad_bound != nullptr);
    if (bounded && !PAIR && !UNIT) mx = __float_as_uint(sp.grad_bound[b]) & 0x7fffffffu;
    float ucoef = 0.0f;
    if constexpr (UNIT) ucoef = st_unit_coef(sp, b, unit, mx);
    if constexpr (PAIR) {
        st_pair_pass1<WORK, CRIT>(sp, b, part, G, n_hits, T, tile_at, mx);
        __threadfence_block();  // the stash is read back by other waves of this workgroup after the barrier below
    }
    for (int h = part * ST_WAVES + wave; h < n_hits && !bounded; h += G * ST_WAVES) {
        const int t = tile_at(h);
        const int yi = (t / sp.tiles_x) * ST_TH + r, x = (t % sp.tiles_x) * ST_TW + x4;
        if (yi >= is || x >= is) continue;  // partial tile at the image border (rows are multiples of 4 wide)
        float g[4][3];
        st_load_grad<FLOWGRAD>(sp, b, yi, x, g);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) mx = max(mx, __float_as_uint(g[j][ch]) & 0x7fffffffu);
    }
    unsigned bm = 0u;
    // (WORK: the barrier behind the table zeroing waits in front of the first LDS atomic of pass 2, behind the tile's loads)
    if constexpr (UNIT) {
        if (!WORK) __syncthreads();  // table zeroed
        bm = mx;          // (the image's bound: the same in every lane of the workgroup, nothing to reduce)
    } else {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
        if (lane == 0) wmax[wave] = mx;
        __syncthreads();  // table zeroed, maxima visible
#pragma unroll
        for (int k = 0; k < ST_WAVES; k++) bm = max(bm, wmax[k]);
    }
    if (bm == 0u) return;                  // every gradient is +-0: nothing to add (block-uniform)
    const bool finite = bm < 0x7f800000u;  // else: fp32 global atomics, Inf / NaN propagate
    // 4. the scale: terms below 2^ST_FIX_BITS, one bit less per doubling of the workgroup's terms beyond 2^13 (launch_plan.hpp)
    const int shift = st_shift(st_headroom(st_terms(n_hits, part, G)), bm);
    // float -> fixed point by the "magic number" addition, two double-precision instructions per value instead of
    // eight (cvt, ldexp, trunc, ldexp, floor, fma, two conversions: the main pass was bound by them -- 24 values per lane, 8
    // waves per SIMD): v 2^shift + 1.5 x 2^52, rounded to an integer by that very addition, has v's fixed-point value in two's
    // complement in the low 51 bits of its mantissa field and a CONSTANT above them; the raw bit patterns are summed by the
    // 64-bit LDS atomics, the constants pile up above bit 50 and are dropped at the flush (sign extension from bit 50).
    // |terms| < 2^ST_FIX_BITS and at most 2^(ST_SUM_BITS - ST_FIX_BITS) of them per cell: the sum stays inside the field.
    const double fix_scale = ldexp(1.0, shift);
    float* out = p.grad_vcolors + (int64_t)b * p.V * 3;

    // 5. pass 2
    // (WORK: every wave takes a FIRST trip, with or without a tile -- the workgroup's barrier sits inside it, at ONE place for
    // all waves)
    for (int h = part * ST_WAVES + wave, trip = 0; h < n_hits || (WORK && trip == 0); h += G * ST_WAVES, trip++) {
        const bool live = h < n_hits;
        const int t = live ? tile_at(h) : 0;
        const int yi = (t / sp.tiles_x) * ST_TH + r, x = (t % sp.tiles_x) * ST_TW + x4;
        const bool inside = live && yi < is && x < is;
        int4 f4 = make_int4(-1, -1, -1, -1);
        if (inside) f4 = *reinterpret_cast<const int4*>(fim_b + (int64_t)yi * is + x);
        const int fn[4] = {f4.x, f4.y, f4.z, f4.w};
        // (a tile the coverage bytes name holds a covered pixel, and the wave IS the tile: testing here would only put
        // the face-index round trip in front of all the other loads; without coverage bytes every tile is walked)
        if (!sp.tile_hit && __ballot(fn[0] >= 0 || fn[1] >= 0 || fn[2] >= 0 || fn[3] >= 0) == 0ull) continue;
        float g[4][3], w[4][3], zp[4], vz[4][3];
        int vid[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            zp[j] = 1.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) { g[j][k] = 0.0f; w[j][k] = 0.0f; }
        }
        if (inside) {
            st_tile_loads<FLOWGRAD, REC, PAIR, UNIT>(sp, b, yi, x, ucoef, g, w, vid, zp);
            if (REC) {
                // The three (vertex, weight) pairs of a pixel are ROTATED by the lane's row in the tile (mod 3).  A
                // face spans three or four rows, so the lanes above one another hold the same three vertex ids, and the LDS
                // atomics of step k below all hit the same table cell -- 65 % of this kernel's LDS-active cycles were such
                // collisions (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/r05_pmc_summary.txt), the LDS pipe the
                // longest phase of a workgroup.  Rotated, neighbouring rows add to DIFFERENT vertices of the face in the same
                // step (the sum does not care about the order).  SQ_LDS_BANK_CONFLICT 1.59 -> 1.27 M per launch.
                // (by row AND column: horizontally adjacent lanes share a face where it straddles their four-pixel groups.
                // 640 x 640, B = 32, warm: 43.9 us unrotated, 36.7 by row, 33.1 by row + column; at 256 x 256, one tile per
                // wave, the launch is not bound by its LDS pipe and does not change)
                // (the scheduling barrier keeps the rotation from being interleaved with the loads around it: without it
                // the unit scatter and the colour-space form need ~80 VGPRs instead of ~62, six waves per SIMD instead of eight)
                if constexpr (UNIT || !FLOWGRAD) __builtin_amdgcn_sched_barrier(0);
                const int rot = (r + (lane & 7)) % 3;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int a0 = vid[j][0], a1 = vid[j][1], a2 = vid[j][2];
                    const float b0 = w[j][0], b1 = w[j][1], b2 = w[j][2];
                    vid[j][0] = rot == 0 ? a0 : (rot == 1 ? a1 : a2);
                    vid[j][1] = rot == 0 ? a1 : (rot == 1 ? a2 : a0);
                    vid[j][2] = rot == 0 ? a2 : (rot == 1 ? a0 : a1);
                    w[j][0] = rot == 0 ? b0 : (rot == 1 ? b1 : b2);
                    w[j][1] = rot == 0 ? b1 : (rot == 1 ? b2 : b0);
                    w[j][2] = rot == 0 ? b2 : (rot == 1 ? b0 : b1);
                }
            }
        }
        if (!REC) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool won = fn[j] >= 0;
                const bool o = fn[j] >= p.F0;  // reversed copy of face fn - F0
                const int32_t* ix = fidx_b + (int64_t)(won ? (o ? fn[j] - p.F0 : fn[j]) : 0) * 3;
#pragma unroll
                for (int k = 0; k < 3; k++) vid[j][k] = won ? ix[o ? 2 - k : k] : 0;
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) vz[j][k] = fn[j] >= 0 ? verts_b[(int64_t)vid[j][k] * 3 + 2] : 1.0f;
        }
        // (Measured and dropped: forming the fixed-point value from the float's bits with 64-bit integer shifts
        // instead of the double-precision ldexp + conversion -- main pass 5.2 -> 7.6 us per workgroup, the 64-bit shifts and
        // selects are slower than the conversion sequence; summing a lane's consecutive pixels of one face in registers
        // before the LDS atomic -- exact, a third fewer atomics, but 54 -> 82 vector registers: three workgroups per compute
        // unit instead of four, or 92 bytes of scratch when capped.)
        if (WORK && trip == 0) __syncthreads();  // (table zeroed; the one barrier of pass 2, reached by every wave)
        if (!live) break;
        // (the finite / non-finite choice -- block-uniform -- is made ONCE around the 24 additions, not inside each of them: the
        // fixed-point path is straight-line code the compiler can interleave, 48 basic blocks otherwise)
        auto add_all = [&](auto fin) __attribute__((always_inline)) {
        constexpr bool FIN = decltype(fin)::value;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (fn[j] < 0) continue;
            float wgs[3];
            if (REC) {
                wgs[0] = w[j][0]; wgs[1] = w[j][1]; wgs[2] = w[j][2];
            } else {
                float fv[9];
                fv[2] = vz[j][0]; fv[5] = vz[j][1]; fv[8] = vz[j][2];
                float tif[3];
                tex_coords(w[j], zp[j], fv, 2, p.eps, tif);
                // taps pn = 1, 2, 4 are the texels holding the colours of vertices 0, 1, 2
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int pn = 1 << k;
                    float wg = 1.0f;
#pragma unroll
                    for (int q = 0; q < 3; q++) wg *= ((pn >> q) & 1) ? (tif[q] - 0.0f) : (1.0f - (tif[q] - 0.0f));
                    wgs[k] = wg;
                }
            }
            float val[9];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) val[k * 3 + ch] = wgs[k] * g[j][ch];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    if (FLOWGRAD && ch == 2) continue;  // the third plane's gradient is identically zero
                    const float v = val[k * 3 + ch];
                    // (records name the vertex behind tap k themselves; else: the texel layout table)
                    const int vtx = REC ? vid[j][k] : sel3(vid[j][0], vid[j][1], vid[j][2], texel_vertex(p.texel, k, fn[j] >= p.F0));
                    const int cell = vtx * NCH + ch;
                    if constexpr (FIN) {
                        const double d = __builtin_fma((double)v, fix_scale, 6755399441055744.0);
                        if (v != 0.0f) atomicAdd(reinterpret_cast<unsigned long long*>(&vtab[cell]), (unsigned long long)__double_as_longlong(d));
                    } else if (v != 0.0f) {
                        atomicAdd(&out[vtx * 3 + ch], v);
                    }
                }
        }
        };
        if (finite) add_all(std::true_type{}); else add_all(std::false_type{});
    }
    // 6. the flush
    if (!finite) return;  // block-uniform
    __syncthreads();
    st_flush<NCH>(vtab, p.V, shift, out);
}

template <bool FLOWGRAD, bool REC>
__global__ void __launch_bounds__(ST_WAVES * MR_WAVE) scatter_tiles_kernel(ScatterTilesParams sp) {
    scatter_tiles_body<FLOWGRAD, REC, false>(sp);
}

// ... with the pair loss's backward folded into pass 1 (mr_flow_pair_backward_tiles).  Eight waves per SIMD: four of
// these 8-wave workgroups per compute unit, i.e. all 1024 of a 128-image launch resident at once, as for the kernel above.
__global__ void __launch_bounds__(ST_WAVES * MR_WAVE) __attribute__((amdgpu_waves_per_eu(8, 8)))
pair_scatter_tiles_kernel(ScatterTilesParams sp) {
    scatter_tiles_body<true, true, true>(sp);
}
// ... for the l2 criterion (MR_CRITERION_L2: res * res per channel, gradient 2 res)
__global__ void __launch_bounds__(ST_WAVES * MR_WAVE) __attribute__((amdgpu_waves_per_eu(8, 8)))
pair_scatter_tiles_l2_kernel(ScatterTilesParams sp) {
    scatter_tiles_body<true, true, true, false, false, PairCrit::L2>(sp);
}

// ... and with the pair loss's gradient already formed by the forward launch (mr_flow_pair_backward_unit_tiles): the
// scatter alone, its gradient = unit gradient x the image's coefficient, its bound = the forward's maximum x |coefficient|
__global__ void __launch_bounds__(ST_WAVES * MR_WAVE) unit_scatter_listing_kernel(ScatterTilesParams sp) {
    scatter_tiles_body<true, true, false, true, false>(sp);
}
// ... and with the workgroups handed out over the forward's covered-tile lists (WORK; what the step launches since round 5)
__global__ void __launch_bounds__(ST_WAVES * MR_WAVE) unit_scatter_tiles_kernel(ScatterTilesParams sp) {
    scatter_tiles_body<true, true, false, true, true>(sp);
}

}  // namespace mr

using namespace mr;

// fills the gather's fields INSIDE a value-initialised block: its padding bytes are kernel-argument bytes too, and a
// list-initialised temporary leaves them to the stack
static void fill_gather_vc(GatherVCParams& g, const float* verts, const int32_t* fidx, const int32_t* fim, const float* grad_rgb,
                           float* grad_vcolors, int B, int V, int F0, int fill_back, int is, float eps, int texel) {
    g.verts = verts; g.fidx = fidx; g.fim = fim; g.grad_rgb = grad_rgb; g.grad_vcolors = grad_vcolors;
    g.B = B; g.V = V; g.F0 = F0; g.fill_back = fill_back; g.is = is; g.eps = eps; g.texel = texel;
}

extern "C" int mr_render_vc_backward(const float* verts, const int32_t* faces_idx, const int32_t* face_index_map,
                                     const float* weight_map, const float* depth_img, const float* grad_rgb_img,
                                     float* grad_vcolors, int batch_size, int num_verts, int num_faces, int fill_back,
                                     int image_size, float eps, int flags, int texel_layout, mr_stream_t stream) {
    if (batch_size < 0 || num_faces < 0 || num_verts < 0 || image_size <= 0 || !texel_layout_ok(texel_layout)) return MR_ERR_BADARG;
    if (!grad_vcolors && (int64_t)batch_size * num_verts > 0) return MR_ERR_BADARG;
    if (batch_size == 0 || num_verts == 0) return MR_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(grad_vcolors, 0, (size_t)batch_size * num_verts * 3 * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    if (num_faces == 0) return MR_OK;
    if (!verts || !faces_idx || !face_index_map || !grad_rgb_img || !(eps >= 1e-6f)) return MR_ERR_BADARG;
    ScatterVCParams sp{};
    fill_gather_vc(sp.g, verts, faces_idx, face_index_map, grad_rgb_img, grad_vcolors, batch_size, num_verts, num_faces, fill_back, image_size, eps,
                   texel_layout);
    sp.weight = weight_map; sp.depth = depth_img;
    const GatherVCParams& g = sp.g;
    const ScatterVCPlan plan = plan_scatter_vc(batch_size, num_verts, num_faces, image_size, flags);
    if (plan.status != MR_OK) return plan.status;
    if (plan.scatter) {
        sp.rx_n = plan.rx_n; sp.ry_n = plan.ry_n;
        const bool stored = weight_map && depth_img;
        hipLaunchKernelGGL(stored ? scatter_vc_kernel<true> : scatter_vc_kernel<false>, dim3(plan.wgs), dim3(SV_WAVES * MR_WAVE), plan.lds, s,
                           sp);
        MR_CHECK_LAUNCH();
        return MR_OK;
    }
    return launch1d(gather_vc_kernel<0>, plan.gather_threads, s, g);
}

// ---- the tile-scatter launches: mr_render_flow_backward, mr_flow_pair_backward_tiles, mr_flow_pair_backward_unit_tiles ----
// What they share.  The entry point has filled sp.g, sp.weight / tile_hit / vid_map / split / H / W and its own fields; this
// runs the common checks in the entry points' common order, zeroes the output unless MR_FLAG_OUTPUT_ZEROED (the workgroups of
// an image meet in global atomics on a zeroed output), completes sp (tiles_x / tiles_y / groups) and launches `kernel` with
// the colour table's LDS bytes.  `args_ok` / `maps_ok`: the entry point's own checks, which take their turn before the
// memset / behind the num_faces == 0 return.  `pairs`: the images are the two frames of batch_size / 2 pairs.
static int launch_scatter_tiles(ScatterTilesParams& sp, int flags, bool pairs, bool args_ok, bool maps_ok,
                                void (*kernel)(ScatterTilesParams), hipStream_t s) {
    const GatherVCParams& g = sp.g;
    if (g.B < 0 || (pairs && (g.B & 1)) || g.F0 < 0 || g.V < 0 || g.is <= 0 || !texel_layout_ok(g.texel)) return MR_ERR_BADARG;
    if (!g.grad_vcolors && (int64_t)g.B * g.V > 0) return MR_ERR_BADARG;
    if (g.B == 0 || g.V == 0) return MR_OK;
    if (!args_ok) return MR_ERR_BADARG;
    if (!(flags & MR_FLAG_OUTPUT_ZEROED)) {
        hipError_t e = hipMemsetAsync(g.grad_vcolors, 0, (size_t)g.B * g.V * 3 * sizeof(float), s);
        if (e != hipSuccess) return (int)e;
    }
    if (g.F0 == 0) return MR_OK;
    if (!g.fim || !sp.weight || !(g.eps >= 1e-6f) || !maps_ok) return MR_ERR_BADARG;
    const ScatterPlan plan = plan_scatter_tiles(g.B, g.V, g.is, g.grad_rgb != nullptr, pairs);
    if (plan.status != MR_OK) return plan.status;
    sp.tiles_x = plan.tiles_x; sp.tiles_y = plan.tiles_y; sp.groups = plan.groups;
    hipLaunchKernelGGL(kernel, dim3(plan.wgs), dim3(ST_WAVES * MR_WAVE), plan.lds, s, sp);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_render_flow_backward(const float* verts, const int32_t* faces_idx, const int32_t* face_index_map,
                                       const uint32_t* tile_hit, const float* weight_map, const float* depth_img,
                                       const float* grad_rgb_img, const float* grad_flow, const float* mask_pre,
                                       const float* mask_x_lo, const float* mask_x_hi, int split, const float* occl,
                                       int height, int width, float* grad_vcolors, int batch_size, int num_verts,
                                       int num_faces, int fill_back, int image_size, float eps, int flags,
                                       const int32_t* vertex_id_map, int texel_layout, const float* grad_bound,
                                       mr_stream_t stream) {
    const bool flowgrad = grad_rgb_img == nullptr;
    ScatterTilesParams sp{};
    fill_gather_vc(sp.g, verts, faces_idx, face_index_map, grad_rgb_img, grad_vcolors, batch_size, num_verts, num_faces, fill_back, image_size, eps,
                   texel_layout);
    sp.weight = weight_map; sp.depth = depth_img; sp.tile_hit = tile_hit; sp.vid_map = vertex_id_map;
    sp.grad_flow = grad_flow; sp.m_pre = mask_pre; sp.m_x_lo = mask_x_lo; sp.m_x_hi = mask_x_hi; sp.occl = occl;
    sp.split = split; sp.H = height; sp.W = width;
    sp.grad_bound = flowgrad ? grad_bound : nullptr;
    const bool args_ok = !flowgrad || (grad_flow && mask_pre && mask_x_lo && occl && height > 0 && width > 0 && height <= image_size &&
                                       width <= image_size && split >= 0 && split <= batch_size && (split == batch_size || mask_x_hi));
    auto kernel = vertex_id_map ? (flowgrad ? scatter_tiles_kernel<true, true> : scatter_tiles_kernel<false, true>)
                                : (flowgrad ? scatter_tiles_kernel<true, false> : scatter_tiles_kernel<false, false>);
    return launch_scatter_tiles(sp, flags, false, args_ok, vertex_id_map || (verts && faces_idx && depth_img), kernel,
                                (hipStream_t)stream);
}

extern "C" int mr_flow_pair_backward_tiles_crit(const int32_t* face_index_map, const uint32_t* tile_hit, const float* weight_map,
                                                const int32_t* vertex_id_map, const float* flows, const float* image_ref,
                                                const float* image, const float* jitter_ref, const float* jitter,
                                                int jitter_channels, const float* sums, const float* grad_loss_fwd,
                                                const float* grad_loss_bwd, const float* mask_pre, const float* mask_x_lo,
                                                const float* mask_x_hi, const float* occl, float* grad_flow_scratch, int height,
                                                int width, float* grad_vcolors, int batch_size, int num_verts, int num_faces,
                                                int fill_back, int image_size, float eps, float pair_thresh, int flags,
                                                int texel_layout, mr_stream_t stream, int criterion) {
    if (!criterion_ok(criterion)) return MR_ERR_BADARG;
    ScatterTilesParams sp{};
    fill_gather_vc(sp.g, nullptr, nullptr, face_index_map, nullptr, grad_vcolors, batch_size, num_verts, num_faces, fill_back, image_size, eps,
                   texel_layout);
    sp.weight = weight_map; sp.tile_hit = tile_hit; sp.vid_map = vertex_id_map;
    sp.m_pre = mask_pre; sp.m_x_lo = mask_x_lo; sp.m_x_hi = mask_x_hi; sp.occl = occl;
    sp.split = batch_size / 2; sp.H = height; sp.W = width;
    sp.stash = grad_flow_scratch; sp.flow = flows; sp.image_ref = image_ref; sp.image = image; sp.jitter_ref = jitter_ref;
    sp.jitter = jitter; sp.Cj = jitter_channels; sp.sums = sums; sp.gl_fwd = grad_loss_fwd; sp.gl_bwd = grad_loss_bwd;
    sp.pair_thresh = pair_thresh;
    const bool args_ok = flows && image_ref && image && jitter_ref && jitter && sums && grad_loss_fwd && mask_pre && mask_x_lo &&
                         mask_x_hi && occl && grad_flow_scratch && tile_hit && (jitter_channels == 1 || jitter_channels == 3) &&
                         height > 0 && width >= 2 && height <= image_size && width <= image_size &&
                         (int64_t)height * width <= (1LL << 29);
    return launch_scatter_tiles(sp, flags, true, args_ok, vertex_id_map != nullptr,
                                criterion == MR_CRITERION_L2 ? pair_scatter_tiles_l2_kernel : pair_scatter_tiles_kernel, (hipStream_t)stream);
}

extern "C" int mr_flow_pair_backward_tiles(const int32_t* face_index_map, const uint32_t* tile_hit, const float* weight_map,
                                           const int32_t* vertex_id_map, const float* flows, const float* image_ref,
                                           const float* image, const float* jitter_ref, const float* jitter,
                                           int jitter_channels, const float* sums, const float* grad_loss_fwd,
                                           const float* grad_loss_bwd, const float* mask_pre, const float* mask_x_lo,
                                           const float* mask_x_hi, const float* occl, float* grad_flow_scratch, int height,
                                           int width, float* grad_vcolors, int batch_size, int num_verts, int num_faces,
                                           int fill_back, int image_size, float eps, float pair_thresh, int flags,
                                           int texel_layout, mr_stream_t stream) {
    return mr_flow_pair_backward_tiles_crit(face_index_map, tile_hit, weight_map, vertex_id_map, flows, image_ref, image, jitter_ref,
                                            jitter, jitter_channels, sums, grad_loss_fwd, grad_loss_bwd, mask_pre, mask_x_lo,
                                            mask_x_hi, occl, grad_flow_scratch, height, width, grad_vcolors, batch_size, num_verts,
                                            num_faces, fill_back, image_size, eps, pair_thresh, flags, texel_layout, stream,
                                            MR_CRITERION_L1);
}

int mr::launch_unit_scatter_tiles(const UnitScatterArgs& a, hipStream_t s) {
    ScatterTilesParams sp{};
    fill_gather_vc(sp.g, nullptr, nullptr, a.face_index_map, nullptr, a.grad_vcolors, a.batch_size, a.num_verts, a.num_faces, a.fill_back,
                   a.image_size, a.eps, a.texel_layout);
    sp.weight = a.weight_map; sp.tile_hit = a.tile_hit; sp.vid_map = a.vertex_id_map;
    sp.split = a.batch_size / 2; sp.H = a.height; sp.W = a.width;
    sp.unit_grad = a.unit_grad; sp.unit_max = a.unit_grad_max; sp.sums = a.sums; sp.gl_fwd = a.grad_loss_fwd; sp.gl_bwd = a.grad_loss_bwd;
    sp.gl_sum = a.grad_loss_sum; sp.gl_mean = a.grad_mean; sp.mean_div = (float)(a.batch_size / 2); sp.mean_of = a.mean_of;
    // (any of the four incoming gradients makes a call, loss_bwd's alone included: the kernels read each behind its null check,
    // and a direction none of them reaches has a zero coefficient)
    const bool args_ok = a.unit_grad && a.unit_grad_max && a.sums && (a.grad_loss_fwd || a.grad_loss_bwd || a.grad_loss_sum || a.grad_mean) &&
                         a.tile_hit &&
                         a.height > 0 && a.width >= 2 && a.height <= a.image_size && a.width <= a.image_size &&
                         (int64_t)a.height * a.width <= (1LL << 29);
    // (the covered-tile lists need the workgroup split's head room, grid > images: every launch has ST_G or more per image)
    static_assert(ST_G >= 2, "unit_scatter_tiles_kernel splits an image's covered tiles over its workgroups");
    if (a.scatter_work) sp.work = scatter_work_at(const_cast<void*>(a.scatter_work), a.batch_size);
    return launch_scatter_tiles(sp, a.flags, true, args_ok, a.vertex_id_map != nullptr,
                                a.scatter_work ? unit_scatter_tiles_kernel : unit_scatter_listing_kernel, s);
}

extern "C" int mr_flow_pair_backward_unit_tiles(const int32_t* face_index_map, const uint32_t* tile_hit,
                                                const float* weight_map, const int32_t* vertex_id_map, const float* unit_grad,
                                                const float* unit_grad_max, const float* sums, const float* grad_loss_fwd,
                                                const float* grad_loss_bwd, int height, int width, float* grad_vcolors,
                                                int batch_size, int num_verts, int num_faces, int fill_back, int image_size,
                                                float eps, int flags, int texel_layout, const void* scatter_work,
                                                mr_stream_t stream) {
    if (!grad_loss_fwd && (int64_t)batch_size * num_verts > 0) return MR_ERR_BADARG;
    UnitScatterArgs a{};
    a.face_index_map = face_index_map; a.tile_hit = tile_hit; a.weight_map = weight_map; a.vertex_id_map = vertex_id_map;
    a.unit_grad = unit_grad; a.unit_grad_max = unit_grad_max; a.sums = sums; a.grad_loss_fwd = grad_loss_fwd; a.grad_loss_bwd = grad_loss_bwd;
    a.height = height; a.width = width; a.grad_vcolors = grad_vcolors;
    a.batch_size = batch_size; a.num_verts = num_verts; a.num_faces = num_faces; a.fill_back = fill_back; a.image_size = image_size;
    a.eps = eps; a.flags = flags; a.texel_layout = texel_layout; a.scatter_work = scatter_work;
    return launch_unit_scatter_tiles(a, (hipStream_t)stream);
}
