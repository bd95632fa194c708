// raster_bwd.hip -- backward of the rasteriser for gfx950 (MI355X), the upstream-compatible path.
//
// Replaces upstream kernels backward_pixel_map / backward_textures / backward_depth_map
// (/root/reference/meshreg/neurender/rasterize.py:269-315).  The vertex-colour backward of the training path and its
// tile scatter are in raster_bwd_vc.hip; neither file includes the other (the map accessors both use are in mr_common.hpp).
//
// Kernels, in file order:
//   * gather_kernel<IMG,TEX,DEPTH> -- E + F for generic 2x2x2 textures: FACE-PARALLEL GATHER instead of
//     per-pixel global atomics.  Four lanes share a face (one bbox row each), walk its pixel bounding
//     box in face_index_map and, for the pixels it won, recompute barycentrics / sampling weights from
//     the vertices (nothing but face_index_map is read back from the forward) into register
//     accumulators; faces with a very large bbox are walked by the whole wave.  Every output element
//     is written exactly once: no memset, no atomics, deterministic.
//   * textures_atomic_recompute_kernel<IMG>, textures_atomic_stored_kernel, depth_atomic_stored_kernel -- generic texture
//     size / upstream-compatible variants (per-pixel atomics on stored or recomputed sampling weights) behind the
//     five-entry-point API.
//   * pixel_map_kernel<IMG> -- kernel D as upstream walks it, one wave per face, reading the eight
//     planes in place (reference algorithm; no workspace needed).
//   * mark_owners_kernel, mark_owners_scalar_kernel -- one flag per face that owns a pixel (four pixels per thread, or one).
//   * compact_owners_kernel -- flags -> owner list, per-image owner records and the strips' weights; zeroes the rows of the
//     faces that own nothing.
//   * strip_list_kernel -- the strips that have work, listed XCD by XCD, heaviest first.
//   * pixel_map_strip_kernel<IMG, L> -- kernel D by strips of L image lines staged in LDS, fed by the per-image owner
//     records (the default when a workspace is given; see the comment there).
//   * strip_gather_kernel<IMG, L, TEX, DEPTH> -- the strip kernel and the E / F gather of the same call in ONE launch,
//     their workgroups interleaved (image orientation only: mr_render_backward).
//
// Entry points: mr_render_backward_list_workspace_bytes, mr_render_backward_workspace_bytes, mr_backward_pixel_map,
// mr_backward_textures, mr_backward_depth_map, mr_render_backward, mr_pixel_map_terms (with its device counter).
#include "mr_common.hpp"
#include "launch_plan.hpp"
#include <algorithm>

namespace mr {

// ---------------------------------------------------------------------------------------
// E + F: face-parallel gather (texture size 2)
// ---------------------------------------------------------------------------------------
struct GatherParams {
    const float* faces;
    const int32_t* fim;       // raster orientation
    const float* grad_rgb;    // nullable
    const float* grad_depth;  // nullable
    float* grad_faces;        // nullable
    float* grad_textures;     // nullable (ts == 2 only)
    int B, F, is;
    float eps;
    int accumulate_faces;     // 1: grad_faces already holds the pixel-map term
    // optional list of the faces that own a pixel (compact_owners_kernel): only those are walked, the rows of the
    // others were zeroed when the list was built
    const uint32_t* owners;
    const unsigned* n_owners;
};

template <bool IMG, bool TEX, bool DEPTH>
__device__ __forceinline__ void gather_pixel(const GatherParams& p, const Face& f, int b, int xi, int yi,
                                             float* gt, float* gf) {
    float w[3], zp;
    bary(f, xi, yi, zp, w);
    const int is = p.is;
    if (TEX) {
        float tif[3];
        tex_coords(w, zp, f.v, 2, p.eps, tif);
        float g[3];
#pragma unroll
        for (int c = 0; c < 3; c++) g[c] = p.grad_rgb[idx3<IMG>(b, yi, xi, c, is)];
#pragma unroll
        for (int pn = 0; pn < 8; pn++) {
            // ts == 2 and 0 <= tif < 1: floor is 0, the tap index is the bit pattern of pn
            float wg = 1.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) wg *= ((pn >> k) & 1) ? (tif[k] - 0.0f) : (1.0f - (tif[k] - 0.0f));
            const int isc = ((pn & 1) << 2) | (((pn >> 1) & 1) << 1) | ((pn >> 2) & 1);
#pragma unroll
            for (int c = 0; c < 3; c++) gt[isc * 3 + c] += wg * g[c];
        }
    }
    if (DEPTH) {
        const float gd = p.grad_depth[idx1<IMG>(b, yi, xi, is)];
        const float d2 = zp * zp;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float zk = f.v[3 * k + 2];
            gf[3 * k + 2] += gd * w[k] * d2 / (zk * zk);
        }
        float tmp[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 2; k++)
#pragma unroll
            for (int l = 0; l < 3; l++) tmp[k] += -f.inv[3 * l + k] / f.v[3 * l + 2];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int l = 0; l < 2; l++) gf[3 * k + l] += -gd * tmp[l] * w[k] * d2 * (float)is / 2.0f;
    }
}

// GGL lanes per face: lane `sub` walks bbox rows sub, sub + lanes, ...; the partial sums are combined with shuffles inside
// the lane group (fixed order: deterministic).  Faces whose bbox exceeds GATHER_BIG_GENERIC pixels are walked by the whole
// wave instead.  (GGL: launch_plan.hpp)
constexpr int GATHER_BIG_GENERIC = 1024;  // generic gather (direct accumulation on the wave-cooperative path)

template <bool TEX, bool DEPTH>
__device__ __forceinline__ void gather_store(const GatherParams& p, int64_t i, const float* gt, const float* gf) {
    if (TEX) {
        float4* o = reinterpret_cast<float4*>(p.grad_textures + i * 24);
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = make_float4(gt[4 * k], gt[4 * k + 1], gt[4 * k + 2], gt[4 * k + 3]);
    }
    if (p.grad_faces) {
        if (p.accumulate_faces) {
            // (kernel D's sums are in the row already: ADD to them with fire-and-forget atomics -- a load + add + store would
            // put one more dependent round trip at the end of every wave; one writer per element here, the order of the two
            // kernels' contributions is the stream's)
            if (DEPTH)
#pragma unroll
                for (int k = 0; k < 9; k++)
                    if (gf[k] != 0.0f) unsafeAtomicAdd(&p.grad_faces[i * 9 + k], gf[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) p.grad_faces[i * 9 + k] = DEPTH ? gf[k] : 0.0f;
        }
    }
}

// (`vbid` of `vgrid`: the workgroup's place in the gather's own grid -- blockIdx.x of gridDim.x when it is launched alone,
// a virtual index when its workgroups are interleaved with kernel D's strips in one launch, strip_gather_kernel)
template <bool IMG, bool TEX, bool DEPTH>
__device__ __forceinline__ void gather_body(const GatherParams& p, const unsigned vbid, const unsigned vgrid) {
    constexpr int NT = TEX ? 24 : 1, NF = DEPTH ? 9 : 1;
    // (owner list: the entries in use are the first ones -- plain block order, so that they spread over the XCDs)
    const int64_t gid = (int64_t)(p.owners ? vbid : xcd_remap(vbid, vgrid)) * blockDim.x + threadIdx.x;
    const int64_t slot = gid / GGL;
    const int sub = (int)(gid % GGL);
    const int lane = threadIdx.x & 63;
    // (the list entry is requested TOGETHER with the list's length, not behind the test on it: the list has room for every
    // face, the entry is inside the allocation whatever the length turns out to be -- one dependent round trip less)
    uint32_t own = 0u;
    if (p.owners) own = p.owners[slot];
    const int64_t total = p.owners ? (int64_t)*p.n_owners : (int64_t)p.B * p.F;
    asm volatile("" : "+v"(own));  // (keeps the load in front of the branch)
    if ((gid - threadIdx.x) / GGL >= total) return;  // block-uniform: nothing left in the list
    const bool valid = slot < total;
    const int64_t i = p.owners ? (valid ? (int64_t)own : 0) : slot;
    const int b = valid ? (int)(i / p.F) : 0;
    const int fn = valid ? (int)(i % p.F) : 0;
    const int is = p.is;

    FaceBox bx;
    bx.x0 = 1; bx.x1 = 0; bx.y0 = 1; bx.y1 = 0;
    if (valid) {
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; k++) v[k] = p.faces[i * 9 + k];
        bx = face_box(v, is);
    }
    const bool nonempty = valid && bx.x0 <= bx.x1;
    const int bw = bx.x1 - bx.x0 + 1, bh = bx.y1 - bx.y0 + 1;
    const bool big = nonempty && bw * bh > GATHER_BIG_GENERIC;

    float gt[NT], gf[NF];

    // very large faces first: the whole wave walks the bbox, lane per pixel, butterfly-reduce,
    // the owner lane stores the result straight away
    unsigned long long m_big = __ballot(big && sub == 0);
    while (m_big) {
        const int src = __ffsll((long long)m_big) - 1;
        m_big &= m_big - 1;
        const int x0 = __shfl((int)bx.x0, src), y0 = __shfl((int)bx.y0, src);
        const int w_ = __shfl(bw, src), n = w_ * __shfl(bh, src);
        const int bb = __shfl(b, src), ff = __shfl(fn, src);
        Face fb;
        load_face(p.faces + ((int64_t)bb * p.F + ff) * 9, fb, is);
        const int32_t* fim_b = p.fim + (int64_t)bb * is * is;
#pragma unroll
        for (int k = 0; k < NT; k++) gt[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < NF; k++) gf[k] = 0.0f;
        // lane per column (chunks of 64 columns), rows in groups of 8 with the 8 index-map loads
        // issued back to back (a degenerate face carries a full-screen bbox: 1024 probes per lane)
        (void)n;
        const int h_ = __shfl(bh, src);
        for (int cx = lane; cx < w_; cx += MR_WAVE) {
            const int xi = x0 + cx;
            for (int r = 0; r < h_; r += 8) {
                int hit[8];
#pragma unroll
                for (int u = 0; u < 8; u++) hit[u] = fim_b[min(y0 + r + u, y0 + h_ - 1) * is + xi];
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (r + u < h_ && hit[u] == ff) gather_pixel<IMG, TEX, DEPTH>(p, fb, bb, xi, y0 + r + u, gt, gf);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            if (TEX)
#pragma unroll
                for (int k = 0; k < NT; k++) gt[k] += __shfl_xor(gt[k], off);
            if (DEPTH)
#pragma unroll
                for (int k = 0; k < NF; k++) gf[k] += __shfl_xor(gf[k], off);
        }
        if (lane == src) gather_store<TEX, DEPTH>(p, (int64_t)bb * p.F + ff, gt, gf);
    }

#pragma unroll
    for (int k = 0; k < NT; k++) gt[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < NF; k++) gf[k] = 0.0f;
    if (nonempty && !big) {
        Face f;
        load_face(p.faces + i * 9, f, is);
        const int32_t* fim_b = p.fim + (int64_t)b * is * is;
        // Round 5.  The face's box goes by chunks of GGL rows x 4 columns: lane `sub` probes row `sub` of the chunk (four
        // probes in flight), the group ORs its lanes' results into one 32-bit mask, and the pixels the face WON are then
        // dealt out over the group's lanes by rank -- the few-pixel faces of a dense mesh win 4.6 of the 14 pixels of
        // their box, so one trip through the ~250 instructions of a pixel serves a whole face at more than half of the
        // lanes, where "every lane walks its own row" ran four trips (one per column) at a sixth of them.
        for (int yc = bx.y0; yc <= bx.y1; yc += GGL)
            for (int xc = bx.x0; xc <= bx.x1; xc += 4) {
                const int yi = yc + sub;
                const int yl = min(yi, (int)bx.y1);
                int hit[4];
#pragma unroll
                for (int u = 0; u < 4; u++) hit[u] = fim_b[yl * is + min(xc + u, (int)bx.x1)];
                unsigned gm = 0u;
#pragma unroll
                for (int u = 0; u < 4; u++) gm |= (yi <= bx.y1 && xc + u <= bx.x1 && hit[u] == fn) ? (1u << (sub * 4 + u)) : 0u;
#pragma unroll
                for (int off = 1; off < GGL; off <<= 1) gm |= (unsigned)__shfl_xor((int)gm, off);
                const int won = __popc(gm);
                for (int r = sub; r < won; r += GGL) {
                    unsigned m = gm;
                    for (int k = 0; k < r; k++) m &= m - 1u;  // drop the r lowest set bits
                    const int pos = __ffs((int)m) - 1;
                    gather_pixel<IMG, TEX, DEPTH>(p, f, b, xc + (pos & 3), yc + (pos >> 2), gt, gf);
                }
            }
    }
    // quad reduction: afterwards every lane of the quad holds the face's sums
#pragma unroll
    for (int off = 1; off < GGL; off <<= 1) {
        if (TEX)
#pragma unroll
            for (int k = 0; k < NT; k++) gt[k] += __shfl_xor(gt[k], off);
        if (DEPTH)
#pragma unroll
            for (int k = 0; k < NF; k++) gf[k] += __shfl_xor(gf[k], off);
    }
    if (valid && sub == 0 && !big) gather_store<TEX, DEPTH>(p, i, gt, gf);
}
template <bool IMG, bool TEX, bool DEPTH>
__global__ void __launch_bounds__(256) gather_kernel(GatherParams p) {
    gather_body<IMG, TEX, DEPTH>(p, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------
// E, generic texture size: per-pixel atomics on recomputed sampling weights
// ---------------------------------------------------------------------------------------
template <bool IMG>
__global__ void __launch_bounds__(256) textures_atomic_recompute_kernel(
    const float* __restrict__ faces, const int32_t* __restrict__ fim, const float* __restrict__ grad_rgb,
    float* __restrict__ grad_textures, int64_t npx, int F, int is, int ts, float eps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const int fn = fim[i];
    if (fn < 0) return;
    const int b = (int)(i / ((int64_t)is * is));
    const int pn_ = (int)(i % ((int64_t)is * is));
    const int yi = pn_ / is, xi = pn_ % is;
    Face f;
    load_face(faces + ((int64_t)b * F + fn) * 9, f, is);
    float w[3], zp, tif[3];
    bary(f, xi, yi, zp, w);
    tex_coords(w, zp, f.v, ts, eps, tif);
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; c++) g[c] = grad_rgb[idx3<IMG>(b, yi, xi, c, is)];
    float* gt = grad_textures + ((int64_t)b * F + fn) * ts * ts * ts * 3;
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        float wg; int isc;
        tex_tap(tif, pn, ts, wg, isc);
#pragma unroll
        for (int c = 0; c < 3; c++) atomicAdd(&gt[isc * 3 + c], wg * g[c]);
    }
}

// upstream backward_textures on stored sampling maps (raster NHWC)
__global__ void __launch_bounds__(256) textures_atomic_stored_kernel(
    const int32_t* __restrict__ fim, const float* __restrict__ swgt, const int32_t* __restrict__ sidx,
    const float* __restrict__ grad_rgb, float* __restrict__ grad_textures, int64_t npx, int F, int is,
    int ts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const int fn = fim[i];
    if (fn < 0) return;
    const int64_t b = i / ((int64_t)is * is);
    float* gt = grad_textures + (b * F + fn) * ts * ts * ts * 3;
    const float g[3] = {grad_rgb[i * 3], grad_rgb[i * 3 + 1], grad_rgb[i * 3 + 2]};
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        const float w = swgt[i * 8 + pn];
        const int isc = sidx[i * 8 + pn];
#pragma unroll
        for (int c = 0; c < 3; c++) atomicAdd(&gt[isc * 3 + c], w * g[c]);
    }
}

// upstream backward_depth_map on stored maps (raster orientation)
__global__ void __launch_bounds__(256) depth_atomic_stored_kernel(
    const float* __restrict__ faces, const float* __restrict__ depth_map, const int32_t* __restrict__ fim,
    const float* __restrict__ face_inv_map, const float* __restrict__ weight_map,
    const float* __restrict__ grad_depth, float* __restrict__ grad_faces, int64_t npx, int F, int is) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const int fn = fim[i];
    if (fn < 0) return;
    const int64_t b = i / ((int64_t)is * is);
    const float* face = faces + (b * F + fn) * 9;
    float* gface = grad_faces + (b * F + fn) * 9;
    const float depth = depth_map[i];
    const float d2 = depth * depth;
    const float gd = grad_depth[i];
    const float* inv = face_inv_map + i * 9;
    const float w[3] = {weight_map[i * 3], weight_map[i * 3 + 1], weight_map[i * 3 + 2]};
    const float z[3] = {face[2], face[5], face[8]};
#pragma unroll
    for (int k = 0; k < 3; k++) atomicAdd(&gface[3 * k + 2], gd * w[k] * d2 / (z[k] * z[k]));
    float tmp[2] = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int l = 0; l < 3; l++) tmp[k] += -inv[3 * l + k] / z[l];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int l = 0; l < 2; l++) atomicAdd(&gface[3 * k + l], -gd * tmp[l] * w[k] * d2 * (float)is / 2.0f);
}

// ---------------------------------------------------------------------------------------
// D: NMR pixel-map pseudo-gradient.
// ---------------------------------------------------------------------------------------
struct PixelMapParams {
    const float* faces;
    const int32_t* fim;  // raster orientation
    const float* rgb;
    const float* alpha;
    const float* grad_rgb;
    const float* grad_alpha;
    float* grad_faces;
    int B, F, is;
    float eps;
    int return_rgb, return_alpha;
    int write_backfacing;  // fused path: also zero the rows of culled faces
    int count_terms;       // MR_FLAG_COUNT_PIXEL_MAP_TERMS: count the walk's terms (mr_pixel_map_terms)
    float* zero_textures;  // nullable: [B*F, 24] texture-gradient rows, zeroed for the faces that own no pixel
    int zero_owner_rows;   // compact_owners_kernel: zero the grad_faces rows of the owning faces too (kernel D by strips adds into them)
};

template <bool IMG>
__device__ __forceinline__ float diff_grad_at(const PixelMapParams& p, int b, int yi, int xi, float a_ref,
                                              const float* rgb_ref) {
    float d = 0.0f;
    const int is = p.is;
    if (p.return_alpha) {
        const int64_t ia = idx1<IMG>(b, yi, xi, is);
        d += (p.alpha[ia] - a_ref) * p.grad_alpha[ia];
    }
    if (p.return_rgb) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int64_t ic = idx3<IMG>(b, yi, xi, k, is);
            d += (p.rgb[ic] - rgb_ref[k]) * p.grad_rgb[ic];
        }
    }
    return d;
}

// One WAVE per face.  The edge / axis / column loops of upstream's per-face walk are wave-uniform
// (every lane evaluates the same scalars); the pixel sweeps along d1 -- up to the image border for
// the "out" sweep -- are spread over the 64 lanes, each lane accumulating partial sums for the six
// (vertex, component) slots, combined by one butterfly reduction at the end.
template <bool IMG>
__global__ void __launch_bounds__(256) pixel_map_kernel(PixelMapParams p) {
    const int64_t total = (int64_t)p.B * p.F;
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // face of this wave
    const int lane = threadIdx.x & 63;
    if (i >= total) return;  // wave-uniform
    const int is = p.is;
    const float fis = (float)is;
    const int b = (int)(i / p.F);
    const int fn = (int)(i % p.F);
    float face[9];
#pragma unroll
    for (int k = 0; k < 9; k++) face[k] = p.faces[i * 9 + k];
    const bool front = !backfacing(face);
    if (!front) {
        if (p.write_backfacing && lane < 9) p.grad_faces[i * 9 + lane] = 0.0f;
        return;
    }
    const int32_t* fim_b = p.fim + (int64_t)b * is * is;
    float acc[3][2];  // [vertex][component] partial sums of this lane
#pragma unroll
    for (int k = 0; k < 3; k++) { acc[k][0] = 0.0f; acc[k][1] = 0.0f; }

#pragma unroll 1
    for (int edge_num = 0; edge_num < 3; edge_num++) {
        int pi[3];
        float pp[3][2];
        for (int num = 0; num < 3; num++) pi[num] = (edge_num + num) % 3;
        for (int num = 0; num < 3; num++)
            for (int dim = 0; dim < 2; dim++) pp[num][dim] = 0.5f * (face[3 * pi[num] + dim] * fis + fis - 1.0f);
#pragma unroll 1
        for (int axis = 0; axis < 2; axis++) {
            float q[3][2];
            for (int num = 0; num < 3; num++)
                for (int dim = 0; dim < 2; dim++) q[num][dim] = pp[num][(dim + axis) % 2];
            int direction;
            if (axis == 0)
                direction = (q[0][0] < q[1][0]) ? -1 : 1;
            else
                direction = (q[0][0] < q[1][0]) ? 1 : -1;
            const int d0_from = (int)fmaxf(ceilf(fminf(q[0][0], q[1][0])), 0.0f);
            const int d0_to = (int)fminf(fmaxf(q[0][0], q[1][0]), fis - 1.0f);
            float g0 = 0.0f, g1 = 0.0f;  // this lane's share for vertices pi[0], pi[1], component 1 - axis
            for (int d0 = d0_from; d0 <= d0_to; d0++) {
                const float fd0 = (float)d0;
                const float d1_cross = (q[1][1] - q[0][1]) / (q[1][0] - q[0][0]) * (fd0 - q[0][0]) + q[0][1];
                const int d1_in = (0 < direction) ? (int)floorf(d1_cross) : (int)ceilf(d1_cross);
                const int d1_out = d1_in + direction;
                if (d1_in < 0 || is <= d1_in) continue;
                if (d1_out < 0 || is <= d1_out) continue;
                // pixel (x, y) of (d0, d1): axis 0 -> (d0, d1), axis 1 -> (d1, d0)
                const int xin = axis == 0 ? d0 : d1_in, yin = axis == 0 ? d1_in : d0;
                const int xout = axis == 0 ? d0 : d1_out, yout = axis == 0 ? d1_out : d0;
                float a_in = 0.0f, a_out = 0.0f, rgb_in[3] = {0, 0, 0}, rgb_out[3] = {0, 0, 0};
                if (p.return_alpha) {
                    a_in = p.alpha[idx1<IMG>(b, yin, xin, is)];
                    a_out = p.alpha[idx1<IMG>(b, yout, xout, is)];
                }
                if (p.return_rgb)
                    for (int k = 0; k < 3; k++) {
                        rgb_in[k] = p.rgb[idx3<IMG>(b, yin, xin, k, is)];
                        rgb_out[k] = p.rgb[idx3<IMG>(b, yout, xout, k, is)];
                    }
                const float c0 = (q[1][0] - q[0][0]) / (q[1][0] - fd0);
                const float c1 = (q[1][0] - q[0][0]) / (fd0 - q[0][0]);
                const bool use0 = q[1][0] != fd0, use1 = q[0][0] != fd0;

                // out sweep: pixels beyond the edge, away from the face, lanes over d1
                if (fim_b[yin * is + xin] == fn) {
                    const int d1_limit = (0 < direction) ? is - 1 : 0;
                    const int d1_from = max(min(d1_out, d1_limit), 0);
                    const int d1_to = min(max(d1_out, d1_limit), is - 1);
                    for (int d1 = d1_from + lane; d1 <= d1_to; d1 += MR_WAVE) {
                        const int xi = axis == 0 ? d0 : d1, yi = axis == 0 ? d1 : d0;
                        const float dg = diff_grad_at<IMG>(p, b, yi, xi, a_in, rgb_in);
                        if (dg <= 0) continue;
                        if (use0) {
                            float dist = c0 * ((float)d1 - d1_cross) * 2.0f / fis;
                            dist = (0 < dist) ? dist + p.eps : dist - p.eps;
                            g0 -= dg / dist;
                        }
                        if (use1) {
                            float dist = c1 * ((float)d1 - d1_cross) * 2.0f / fis;
                            dist = (0 < dist) ? dist + p.eps : dist - p.eps;
                            g1 -= dg / dist;
                        }
                    }
                }
                // in sweep: this face's pixels between the edge and the opposite boundary
                {
                    float d0_cross2;
                    if ((fd0 - q[0][0]) * (fd0 - q[2][0]) < 0)
                        d0_cross2 = (q[2][1] - q[0][1]) / (q[2][0] - q[0][0]) * (fd0 - q[0][0]) + q[0][1];
                    else
                        d0_cross2 = (q[1][1] - q[2][1]) / (q[1][0] - q[2][0]) * (fd0 - q[2][0]) + q[2][1];
                    const int d1_limit = (0 < direction) ? (int)ceilf(d0_cross2) : (int)floorf(d0_cross2);
                    const int d1_from = max(min(d1_in, d1_limit), 0);
                    const int d1_to = min(max(d1_in, d1_limit), is - 1);
                    for (int d1 = d1_from + lane; d1 <= d1_to; d1 += MR_WAVE) {
                        const int xi = axis == 0 ? d0 : d1, yi = axis == 0 ? d1 : d0;
                        if (fim_b[yi * is + xi] != fn) continue;
                        const float dg = diff_grad_at<IMG>(p, b, yi, xi, a_out, rgb_out);
                        if (dg <= 0) continue;
                        if (use0) {
                            float dist = c0 * ((float)d1 - d1_cross) * 2.0f / fis;
                            dist = (0 < dist) ? dist + p.eps : dist - p.eps;
                            g0 -= dg / dist;
                        }
                        if (use1) {
                            float dist = c1 * ((float)d1 - d1_cross) * 2.0f / fis;
                            dist = (0 < dist) ? dist + p.eps : dist - p.eps;
                            g1 -= dg / dist;
                        }
                    }
                }
            }
            // slot (vertex pi[0], comp 1 - axis) += g0 ; slot (vertex pi[1], comp 1 - axis) += g1
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (k == pi[0]) acc[k][1 - axis] += g0;
                if (k == pi[1]) acc[k][1 - axis] += g1;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            acc[k][0] += __shfl_xor(acc[k][0], off);
            acc[k][1] += __shfl_xor(acc[k][1], off);
        }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            p.grad_faces[i * 9 + 3 * k + 0] = acc[k][0];
            p.grad_faces[i * 9 + 3 * k + 1] = acc[k][1];
            p.grad_faces[i * 9 + 3 * k + 2] = 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------
// D by strips: helpers
// ---------------------------------------------------------------------------------------
constexpr int PM_LONG = 12;  // "in" sweeps longer than this are cut into chunk tasks, shorter ones are walked by the lane that found them

// one accepted term of a walk: -dg / (c * (d1 - d1_cross) * 2 / is +- eps), with the two divisions
// done as multiplications by reciprocals (v_rcp_f32, 1 ulp): the walks evaluate > 10^8 of these per
// launch and an IEEE division is ten instructions
__device__ __forceinline__ float pm_term(float dg, float c, float fd1, float d1_cross, float two_over_is, float eps) {
    float dist = (c * two_over_is) * (fd1 - d1_cross);  // c * two_over_is is loop-invariant
    dist = (0 < dist) ? dist + eps : dist - eps;
    return dg * __builtin_amdgcn_rcpf(dist);
}
// owns[b * F + face] = 1 for every face that won a pixel (four pixels per thread)
// (`zero` / `n_zero`: a word array cleared on the way -- the strip weights of kernel D, which the next kernel adds into)
__global__ void __launch_bounds__(256) mark_owners_kernel(const int32_t* __restrict__ fim, uint8_t* __restrict__ owns,
                                                          int64_t npx4, int64_t px_per_image, int F,
                                                          unsigned* __restrict__ zero, int64_t n_zero) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_zero) zero[i] = 0u;
    if (i >= npx4) return;
    const int4 f = reinterpret_cast<const int4*>(fim)[i];
    uint8_t* o = owns + ((i * 4) / px_per_image) * F;
    if (f.x >= 0) o[f.x] = 1;
    if (f.y >= 0) o[f.y] = 1;
    if (f.z >= 0) o[f.z] = 1;
    if (f.w >= 0) o[f.w] = 1;
}

__global__ void __launch_bounds__(256) mark_owners_scalar_kernel(const int32_t* __restrict__ fim,
                                                                 uint8_t* __restrict__ owns, int64_t npx,
                                                                 int64_t px_per_image, int F,
                                                                 unsigned* __restrict__ zero, int64_t n_zero) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_zero) zero[i] = 0u;
    if (i >= npx) return;
    const int f = fim[i];
    if (f >= 0) owns[(i / px_per_image) * F + f] = 1;
}

// the sum of a value over the wave, valid in lane 63: row shifts and the two row broadcasts of the gfx9 DPP unit
// (six VALU instructions, no LDS crossbar)
__device__ __forceinline__ float wave_sum_last(float v) {
    auto step = [](float x, auto ctrl, auto row_mask) {
        return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, decltype(row_mask)::value, 0xf, false));
    };
    v = step(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});  // row_shr:1
    v = step(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});  // row_shr:2
    v = step(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});  // row_shr:4
    v = step(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});  // row_shr:8 -> lane 15 of a row = the row
    v = step(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});  // row_bcast:15 into rows 1, 3
    v = step(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});  // row_bcast:31 into rows 2, 3
    return v;
}
// the maximum of a non-negative value over the wave, valid in lane 63
__device__ __forceinline__ float wave_max_last(float v) {
    auto step = [](float x, auto ctrl, auto row_mask) {
        return fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, decltype(row_mask)::value, 0xf, false)));
    };
    v = step(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
    v = step(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
    v = step(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
    v = step(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
    v = step(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
    v = step(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
    return v;
}

// The faces that own a pixel (typically a fifth of them), compacted into a list for the gather / the walk kernel; the
// others get their zero rows here.  One workgroup per image and CO_TPB * CO_PER faces of it, ONE global atomic each (two with
// `img_recs`: the front-facing ones once more image by image, [B][F] records of two float4 -- the vertices in pixel
// coordinates, 0.5 * (v * is + is - 1) as kernel D computes them, and the face number -- with the counts in
// img_count[b] and the range of lines their crossings can fall on in img_count[B + 4 b ..]: kernel D by strips walks
// the owners of ONE image and reads nothing else of a face).
// faces per thread: 1 -- seven workgroups per image of the bench meshes instead of two; most of this kernel's time is the zero
// rows it writes (60 MB per launch at the metric config), which 128 workgroups do not stream at the chip's rate: 17.8 -> 13.8 us
__global__ void __launch_bounds__(CO_TPB) compact_owners_kernel(PixelMapParams p, const uint8_t* __restrict__ owns,
                                                                unsigned* __restrict__ counter, uint32_t* __restrict__ list,
                                                                unsigned* __restrict__ img_count, float4* __restrict__ img_recs,
                                                                int chunks, unsigned* __restrict__ strip_w, int strip_l,
                                                                int strips_axis) {
    __shared__ unsigned s_cnt, s_base, s_icnt, s_ibase, s_range[4];
    __shared__ uint8_t s_own[CO_TPB * CO_PER];
    constexpr int CO_WMAX = 2048;         // strip weights of the image gathered in LDS first (2 * strips_axis <= CO_WMAX)
    __shared__ unsigned s_w[CO_WMAX];
    const bool lds_w = strip_w != nullptr && 2 * strips_axis <= CO_WMAX;
    if (lds_w)
        for (int q = threadIdx.x; q < 2 * strips_axis; q += CO_TPB) s_w[q] = 0u;
    const int b = blockIdx.x / chunks, fc0 = (blockIdx.x % chunks) * (CO_TPB * CO_PER);
    const int nf = min(CO_TPB * CO_PER, p.F - fc0);  // faces of this workgroup
    const int64_t f0 = (int64_t)b * p.F + fc0;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) { s_cnt = 0u; s_icnt = 0u; }
    if (tid < 4) s_range[tid] = 0u;
    __syncthreads();
    unsigned pos[CO_PER], ipos[CO_PER];
    bool own[CO_PER], iown[CO_PER];
    float pxy[CO_PER][6];
#pragma unroll
    for (int k = 0; k < CO_PER; k++) {
        iown[k] = false; ipos[k] = 0u;
        const int q = k * CO_TPB + tid;
        const int64_t i = f0 + q;
        own[k] = q < nf && owns[i] != 0;
        // bit 0: owns a pixel; bit 1: its grad_faces row is to be zeroed here
        const bool zero_row = q < nf && (!own[k] || p.zero_owner_rows) && p.grad_faces &&
                              (p.write_backfacing || !backfacing(p.faces + i * 9));
        s_own[q] = (own[k] ? 1 : 0) | (zero_row ? 2 : 0);
        const unsigned long long m = __ballot(own[k]);
        unsigned wbase = 0u;
        if (lane == 0 && m) wbase = atomicAdd(&s_cnt, (unsigned)__popcll(m));
        pos[k] = (unsigned)__shfl((int)wbase, 0) + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (img_recs) {
            // the record, and the lines (columns, rows) the crossings of the face can fall on: the union over its edges
            // of kernel D's d0 ranges, kept per image as {max d0_to + 1, is - min d0_from} per axis (0 = none)
            const float fis = (float)p.is;
            float f9[9];
#pragma unroll
            for (int c = 0; c < 9; c++) f9[c] = own[k] ? p.faces[i * 9 + c] : 0.0f;
            iown[k] = own[k] && !backfacing(f9);
#pragma unroll
            for (int v = 0; v < 3; v++) {
                pxy[k][2 * v] = 0.5f * (f9[3 * v] * fis + fis - 1.0f);
                pxy[k][2 * v + 1] = 0.5f * (f9[3 * v + 1] * fis + fis - 1.0f);
            }
            float hi[2] = {0.0f, 0.0f}, lo[2] = {0.0f, 0.0f};
#pragma unroll
            for (int axis = 0; axis < 2; axis++) {
                const float q0 = pxy[k][axis], q1 = pxy[k][2 + axis], q2 = pxy[k][4 + axis];
                const int from = (int)fmaxf(ceilf(fminf(fminf(q0, q1), q2)), 0.0f);
                const int to = (int)fminf(fmaxf(fmaxf(q0, q1), q2), fis - 1.0f);
                if (iown[k] && from <= to) {
                    hi[axis] = (float)(to + 1); lo[axis] = (float)(p.is - from);
                    // ... and, strip by strip, how many owners have crossings there: the strips' weights (strip_list_kernel)
                    if (strip_w)
                        for (int sx = from / strip_l; sx <= to / strip_l; sx++) {
                            if (lds_w) atomicAdd(&s_w[axis * strips_axis + sx], 1u);
                            else atomicAdd(&strip_w[((int64_t)b * 2 + axis) * strips_axis + sx], 1u);
                        }
                }
            }
            const unsigned long long mi = __ballot(iown[k]);
            if (mi) {  // (wave-uniform)
                const float r0 = wave_max_last(hi[0]), r1 = wave_max_last(lo[0]), r2 = wave_max_last(hi[1]), r3 = wave_max_last(lo[1]);
                unsigned ibase = 0u;
                if (lane == 63) {
                    ibase = atomicAdd(&s_icnt, (unsigned)__popcll(mi));
                    atomicMax(&s_range[0], (unsigned)r0); atomicMax(&s_range[1], (unsigned)r1);
                    atomicMax(&s_range[2], (unsigned)r2); atomicMax(&s_range[3], (unsigned)r3);
                }
                ipos[k] = (unsigned)__shfl((int)ibase, 63) + (unsigned)__popcll(mi & ((1ull << lane) - 1ull));
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        s_base = atomicAdd(counter, s_cnt);
        if (img_recs) s_ibase = atomicAdd(&img_count[b], s_icnt);
    }
    if (img_recs && tid < 4 && s_range[tid]) atomicMax(&img_count[p.B + 4 * b + tid], s_range[tid]);
    if (lds_w)
        for (int q = tid; q < 2 * strips_axis; q += CO_TPB)
            if (s_w[q]) atomicAdd(&strip_w[(int64_t)b * 2 * strips_axis + q], s_w[q]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CO_PER; k++)
        if (own[k]) {
            list[s_base + pos[k]] = (uint32_t)(f0 + k * CO_TPB + tid);
            if (iown[k]) {
                float4* rec = img_recs + 2 * ((int64_t)b * p.F + s_ibase + ipos[k]);
                rec[0] = make_float4(pxy[k][0], pxy[k][1], pxy[k][2], pxy[k][3]);
                rec[1] = make_float4(pxy[k][4], pxy[k][5], __int_as_float(fc0 + k * CO_TPB + tid), 0.0f);
            }
        }
    // the zero rows of the workgroup's faces (36 bytes of grad_faces, 96 bytes of texture gradient), consecutive
    // lanes on consecutive addresses
    if (p.grad_faces) {
        float* rows = p.grad_faces + f0 * 9;
        for (int q = tid; q < nf * 9; q += CO_TPB)
            if (s_own[q / 9] & 2) rows[q] = 0.0f;
    }
    if (p.zero_textures) {
        float4* rows = reinterpret_cast<float4*>(p.zero_textures + f0 * 24);
        for (int q = tid; q < nf * 6; q += CO_TPB)
            if (!(s_own[q / 6] & 1)) rows[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ---------------------------------------------------------------------------------------
// D by STRIPS: the sweeps read the maps from LDS, every map byte is fetched once per axis
// ---------------------------------------------------------------------------------------
// The walks of kernel D are sweeps along image columns (axis 0) and rows (axis 1): 1.5 x 10^8 terms per launch of the
// bench workload, every term the eight map values of a pixel.  Walking face by face (pixel_map_kernel; rounds 1-2 also
// on two packed copies of the maps, 2 x 32 B per pixel of workspace and a pack pass in front) re-reads a line once per
// face that crosses it -- dozens of times -- from L2 or beyond.  Here a workgroup OWNS a strip of L adjacent lines of
// one image and one axis: it stages the strip's values in LDS once (for axis 0 straight from the planes, L * 4 bytes
// per image row: the other columns of those cache lines are the neighbouring strips', which run next to it on the same
// XCD -- all strips of an image do, blockIdx -> (image, strip) below -- so they come from that XCD's L2), lists the
// (face, edge) pairs of the image's owning faces whose crossings fall into the strip, and runs their sweeps out of LDS.
//   * owners: compact_owners_kernel leaves, per image, the front-facing owners as records of pixel-space vertices and
//     the range of lines their crossings can fall on; a strip outside the range returns after one load;
//   * enumeration: a thread per owner, 256 a round (the records of the first rounds requested before the strip is
//     staged, all of a workgroup's global loads in flight together), entries (owner | edge | first line | lines - 1)
//     appended to an LDS queue, flushed when another round might not fit;
//   * waves take batches of 64 / L entries, one LANE per (entry, line): crossing, "in" / "out" pixels, short "in"
//     sweep -- the per-item header of upstream's walk, same arithmetic;
//   * the "out" sweeps and the long "in" sweeps are cut into chunks of 16 positions and handed out one per LANE: the
//     lane fetches its item's header from the lane that computed it (ds_bpermute) and walks the chunk by itself, its
//     start rotated so that the 16 lanes of a ds_read_b128 group never share a bank; two positions' values requested
//     while the previous two are worked on; both distances of a term in packed fp32 and one v_rcp_f32 for the two;
//   * sums: a workgroup contributes to ONE component (1 - axis) of a face's three vertices: chunk sums meet in LDS
//     atomics per item, the lines of an entry in a shuffle, one pair of global atomic adds per entry (rows zeroed by
//     compact_owners_kernel).  Float atomics: the order of the additions across chunks and strips is not fixed -- as
//     for the texture / depth terms of this backward pass upstream; MR_FLAG_REFERENCE_ALGO keeps the ordered walk.
// Measured (B = 64, 256 x 256, 3076 faces, MI355X): 310 us + 21 us (owner records) + 6 us (flags), against 425 us
// + 95 us (pack) + 15 us of the packed per-face walk; ~70 % of it is VALU issue of the 1.5 x 10^8 terms (31
// instructions a term), the rest the per-strip phases that wait on memory.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// sum over the channels of (value - reference) * gradient: v = (alpha, r, g, b), g = their gradients (channels a launch
// does not render are staged as zeros); two packed subtractions, a packed multiply and a packed fma
__device__ __forceinline__ float ps_diff_grad(const float4 v, const float4 g, const float4 ref) {
#pragma clang fp contract(fast)  // D is compared to 1e-4, not bit for bit
    const f32x2 v0 = {v.x, v.y}, v1 = {v.z, v.w}, r0 = {ref.x, ref.y}, r1 = {ref.z, ref.w};
    const f32x2 g0 = {g.x, g.y}, g1 = {g.z, g.w};
    const f32x2 d = (v0 - r0) * g0 + (v1 - r1) * g1;
    return d.x + d.y;
}
__device__ __forceinline__ float ps_bound_k(float k) { return (k == k) ? fminf(fmaxf(k, -1e15f), 1e15f) : k; }
// Terms of the walk (MR_FLAG_COUNT_PIXEL_MAP_TERMS; read back by mr_pixel_map_terms): one term = one evaluation of upstream's
// sweep body (rasterize.py:269-281 -> backward_pixel_map: every position of an "out" sweep, every position of an "in" sweep whose
// pixel belongs to the face) -- the unit bench.py's `d_e_f.frac_of_algorithmic_issue` prices at 10 lane-instructions.
__device__ unsigned long long mr_pixel_map_terms_counter;
__device__ __forceinline__ void ps_count_terms(int n) {
    int tot = n;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) tot += __shfl_xor(tot, off);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(&mr_pixel_map_terms_counter, (unsigned long long)tot);
}
// (PS_T threads, PS_QCAP queued entries, PS_TASKS chunk tasks, the lines per strip and the strip kernel's LDS bytes: launch_plan.hpp)

// The strips that have work, XCD by XCD (image b runs on XCD b % 8: all strips of an image behind one L2), HEAVIEST FIRST.
// One workgroup per XCD reads the weights compact_owners_kernel left (owners with crossings per strip), and lists the
// strips with a non-zero weight in three classes -- at least half / a quarter of the largest weight, the rest.  The
// strip kernel takes workgroup i = entry i / 8 of XCD i % 8: no workgroup for the 57 % of the strips outside their image's
// line range (each used to hold one of the chip's 768 slots for a microsecond or two), and the strips through the middle
// of the meshes (up to 100 us each) start first instead of wherever the image order put them (workgroup timeline,
// profiles/r03_kernel_d.txt: last start 265 us into a 315 us launch, 650-700 working strips resident of 768).
__global__ void __launch_bounds__(SL_T) strip_list_kernel(const unsigned* __restrict__ strip_w, unsigned* __restrict__ lists,
                                                          unsigned* __restrict__ counts, int B, int S, int cap) {
    __shared__ unsigned s_max, s_n[3], s_at[3];
    const int x = blockIdx.x, tid = threadIdx.x;
    const int n_img = (B - x + 7) / 8;  // images x, x + 8, ...
    const int total = n_img * S;
    if (tid == 0) { s_max = 0u; s_n[0] = s_n[1] = s_n[2] = 0u; }
    __syncthreads();
    unsigned mx = 0u;
    for (int i = tid; i < total; i += SL_T) mx = max(mx, strip_w[(int64_t)((i / S) * 8 + x) * S + i % S]);
    if (mx) atomicMax(&s_max, mx);
    __syncthreads();
    const unsigned hi = s_max / 2u, mid = s_max / 4u;
    auto cls = [&](unsigned w) { return w > hi ? 0 : (w > mid ? 1 : 2); };
    for (int i = tid; i < total; i += SL_T) {
        const unsigned w = strip_w[(int64_t)((i / S) * 8 + x) * S + i % S];
        if (w) atomicAdd(&s_n[cls(w)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        s_at[0] = 0u; s_at[1] = s_n[0]; s_at[2] = s_n[0] + s_n[1];
        counts[x] = s_n[0] + s_n[1] + s_n[2];
    }
    __syncthreads();
    unsigned* out = lists + (int64_t)x * cap;
    for (int i = tid; i < total; i += SL_T) {
        const int b = (i / S) * 8 + x;
        const unsigned w = strip_w[(int64_t)b * S + i % S];
        if (w) out[atomicAdd(&s_at[cls(w)], 1u)] = (unsigned)(b * S + i % S);
    }
}

template <bool IMG, int L>
__device__ __forceinline__ void strip_body(const PixelMapParams& p, const unsigned* __restrict__ img_count,
                                           const float4* __restrict__ img_recs, int strips_axis,
                                           const unsigned* __restrict__ strip_lists,
                                           const unsigned* __restrict__ strip_counts, int list_cap, const unsigned vbid) {
    extern __shared__ float4 ps_lds[];
    __shared__ unsigned s_qn, s_next;
    constexpr int ENT = MR_WAVE / L;  // entries per batch of a wave
    const int is = p.is, stride = is + 1;  // (+1: the L lines of a staging store fall into different banks)
    float4* recA = ps_lds;                 // [L][stride]  alpha, r, g, b
    float4* recB = recA + L * stride;      // [L][stride]  d alpha, d r, d g, d b
    int* fimL = reinterpret_cast<int*>(recB + L * stride);  // [L][stride]  face index map
    unsigned* queue = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(fimL) + ((L * stride * 4 + 15) & ~15));
    unsigned* sweeps = queue + PS_QCAP;  // (the task lists and the per-item sums of the waves)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx -> XCD blockIdx % 8: every strip of an image on the same XCD; entry blockIdx / 8 of that XCD's list of
    // working strips (heaviest first), `b * S + axis * strips_axis + strip`
    // (vbid: blockIdx.x, or the strip's virtual index when the launch also carries the gather's workgroups -- same residue mod 8)
    const unsigned S = 2u * (unsigned)strips_axis, xcd = vbid & 7u, j = vbid >> 3;
    if (j >= strip_counts[xcd]) return;
    const unsigned ent = strip_lists[(int64_t)xcd * list_cap + j];
    const int b = (int)(ent / S);
    const unsigned sidx = ent % S;
    const int axis = (int)(sidx / (unsigned)strips_axis), l0 = (int)(sidx % (unsigned)strips_axis) * L;
    const int nl = min(L, is - l0);
    const bool ra = p.return_alpha != 0, rr = p.return_rgb != 0;
    const float fis = (float)is, two_over_is = 2.0f / fis;
    const int32_t* fim_b = p.fim + (int64_t)b * is * is;

    auto stage = [&](int line, int d1) {
        const int x = axis == 0 ? l0 + line : d1, y = axis == 0 ? d1 : l0 + line;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ra) {
            const int64_t ia = idx1<IMG>(b, y, x, is);
            v[0] = p.alpha[ia]; v[1] = p.grad_alpha[ia];
        }
        if (rr) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int64_t ic = idx3<IMG>(b, y, x, k, is);
                v[2 + k] = p.rgb[ic]; v[5 + k] = p.grad_rgb[ic];
            }
        }
        recA[line * stride + d1] = make_float4(v[0], v[2], v[3], v[4]);
        recB[line * stride + d1] = make_float4(v[1], v[5], v[6], v[7]);
        fimL[line * stride + d1] = fim_b[y * is + x];
    };
    auto stage_strip = [&]() {
        if (axis == 0) {
            for (int idx = tid; idx < L * is; idx += PS_T)
                if ((idx % L) < nl) stage(idx % L, idx / L);
        } else {
            for (int line = 0; line < nl; line++)
                for (int d1 = tid; d1 < is; d1 += PS_T) stage(line, d1);
        }
    };
    if (tid == 0) { s_qn = 0u; s_next = 0u; }
    const unsigned n_own = img_count[b];
    const float4* own_b = img_recs + 2 * (int64_t)b * p.F;

    const int comp = 1 - axis;
    uint16_t* tasks = reinterpret_cast<uint16_t*>(sweeps) + wave * PS_TASKS;
    float2* acc = reinterpret_cast<float2*>(reinterpret_cast<uint16_t*>(sweeps) + (PS_T / MR_WAVE) * PS_TASKS) + wave * MR_WAVE;
    // a sweep is cut into chunks of CH positions (a power of two >= is / 16: at most 16 chunks per sweep; short chunks
    // fill the lanes of the task rounds: a batch of 64 items has a few hundred)
    int CH = 16;
    while (CH * 16 < is) CH <<= 1;

    auto process = [&](unsigned qn) {
#pragma unroll 1
        for (;;) {
            unsigned base = 0u;
            if (lane == 0) base = atomicAdd(&s_next, (unsigned)ENT);
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            if (base >= qn) break;
            const unsigned ei = base + (unsigned)(lane / L);
            const int loff = lane % L;
            const bool have = ei < qn;
            const unsigned ent = have ? queue[ei] : 0u;
            const int slot = (int)(ent & 0xffffffu), e = (int)((ent >> 24) & 3u);
            const int lfirst = (int)((ent >> 26) & 3u), lcnt = (int)((ent >> 28) & 3u);
            bool valid = have && loff <= lcnt;
            const int line = min(lfirst + loff, L - 1), d0 = l0 + line;
            const float4 v01 = own_b[2 * slot], v2n = own_b[2 * slot + 1];
            const float px[3] = {v01.x, v01.z, v2n.x}, py[3] = {v01.y, v01.w, v2n.y};
            const int fn = __float_as_int(v2n.z);
            const int64_t i = (int64_t)b * p.F + fn;
            // q[num]: vertices e, e+1, e+2, the coordinate pair swapped for axis 1
            float qx[3], qy[3];
#pragma unroll
            for (int num = 0; num < 3; num++) {
                const float vx = (e == 0) ? px[num] : ((e == 1) ? px[(num + 1) % 3] : px[(num + 2) % 3]);
                const float vy = (e == 0) ? py[num] : ((e == 1) ? py[(num + 1) % 3] : py[(num + 2) % 3]);
                qx[num] = axis == 0 ? vx : vy;
                qy[num] = axis == 0 ? vy : vx;
            }
            const int direction = (axis == 0) ? ((qx[0] < qx[1]) ? -1 : 1) : ((qx[0] < qx[1]) ? 1 : -1);
            const float fd0 = (float)d0;
            const float d1_cross = (qy[1] - qy[0]) / (qx[1] - qx[0]) * (fd0 - qx[0]) + qy[0];
            const int d1_in = (0 < direction) ? (int)floorf(d1_cross) : (int)ceilf(d1_cross);
            const int d1_out = d1_in + direction;
            valid = valid && !(d1_in < 0 || is <= d1_in) && !(d1_out < 0 || is <= d1_out);
            const int d1_in_c = min(max(d1_in, 0), is - 1), d1_out_c = min(max(d1_out, 0), is - 1);
            const float4 iA = recA[line * stride + d1_in_c], oA = recA[line * stride + d1_out_c];
            const bool visible = valid && fimL[line * stride + d1_in_c] == fn;
            const float a_in = iA.x, a_out = oA.x;
            const float rgb_in[3] = {iA.y, iA.z, iA.w}, rgb_out[3] = {oA.y, oA.z, oA.w};
            const float c0 = (qx[1] - qx[0]) / (qx[1] - fd0);
            const float c1 = (qx[1] - qx[0]) / (fd0 - qx[0]);
            const bool use0 = qx[1] != fd0, use1 = qx[0] != fd0;
            float d0_cross2;
            if ((fd0 - qx[0]) * (fd0 - qx[2]) < 0)
                d0_cross2 = (qy[2] - qy[0]) / (qx[2] - qx[0]) * (fd0 - qx[0]) + qy[0];
            else
                d0_cross2 = (qy[1] - qy[2]) / (qx[1] - qx[2]) * (fd0 - qx[2]) + qy[2];
            const float lim_f = (0 < direction) ? ceilf(d0_cross2) : floorf(d0_cross2);
            const int d1_limit = (lim_f == lim_f) ? (int)fminf(fmaxf(lim_f, -2.0f), fis + 1.0f) : (int)0x80000000;
            const int in_from = max(min(d1_in, d1_limit), 0), in_to = min(max(d1_in, d1_limit), is - 1);
            const bool long_in = valid && (in_to - in_from) >= PM_LONG;

            float g0 = 0.0f, g1 = 0.0f;  // short "in" sweep: the lane walks its own item
            if (valid && !long_in) {
                for (int d1 = in_from; d1 <= in_to; d1++) {
                    if (fimL[line * stride + d1] != fn) continue;
                    const float dg = ps_diff_grad(recA[line * stride + d1], recB[line * stride + d1],
                                                  make_float4(a_out, rgb_out[0], rgb_out[1], rgb_out[2]));
                    if (dg <= 0) continue;
                    if (use0) g0 -= pm_term(dg, c0, (float)d1, d1_cross, two_over_is, p.eps);
                    if (use1) g1 -= pm_term(dg, c1, (float)d1, d1_cross, two_over_is, p.eps);
                }
            }
            if (p.count_terms) {  // (the terms of the short "in" sweeps)
                int nt = 0;
                if (valid && !long_in)
                    for (int d1 = in_from; d1 <= in_to; d1++) nt += fimL[line * stride + d1] == fn ? 1 : 0;
                ps_count_terms(nt);
            }
            acc[lane] = make_float2(0.0f, 0.0f);  // the sums of this lane's item over its chunks (LDS atomics of the task lanes)

            // The "out" sweeps of the visible items and the long "in" sweeps, one LANE per chunk of CH positions.  A lane
            // fetches the header of its chunk's item from the lane that computed it (ds_bpermute) and walks the chunk
            // by itself -- no staging of headers, no sums across lanes -- starting at the position that puts its
            // records on the LDS bank quad of its lane number: base + position = lane (mod 16) for all lanes and steps
            // alike, so the 16 lanes of a ds_read_b128 group never share a bank.
            const float k0 = c0 * two_over_is, k1 = c1 * two_over_is;
            const int lim = (0 < direction) ? is - 1 : 0;
            const int o_from = max(min(d1_out, lim), 0), o_to = min(max(d1_out, lim), is - 1);
            const int hdr = line | (e << 4) | ((0 < direction ? 1 : 0) << 6) | ((use0 ? 1 : 0) << 7) | ((use1 ? 1 : 0) << 8);
            const int r_out = o_from | (o_to << 16), r_in = in_from | (in_to << 16);
#pragma unroll 1
            for (int kind = 0; kind < 2; kind++) {  // 0: "out" sweeps, 1: long "in" sweeps (only this face's pixels)
                const bool want = kind == 0 ? visible : long_in;
                const int span = kind == 0 ? o_to - o_from : in_to - in_from;
                const int n = want ? span / CH + 1 : 0;
                const int incl = (int)wave_sum_last((float)n);  // (inclusive scan; exact: at most 1024)
                const int total = __builtin_amdgcn_readlane(incl, 63);
                if (total == 0) continue;
                for (int c = 0; c < n; c++) tasks[incl - n + c] = (uint16_t)(lane | (c << 6));
                __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                for (int t0 = 0; t0 < total; t0 += MR_WAVE) {
                    const bool mine = t0 + lane < total;
                    const int task = mine ? (int)tasks[t0 + lane] : 0;
                    const int src = task & 63, c = task >> 6;
                    // (the two distances of a term share ONE reciprocal, 1 / (x y): |k| is kept below 1e15 so that the
                    // product stays finite -- an edge that all but touches the line has k up to inf, its terms are 0 in
                    // upstream's dg / dist and < 1e-15 dg here; a NaN stays a NaN)
                    const float t_cross = __shfl(d1_cross, src), t_k0 = ps_bound_k(__shfl(k0, src)), t_k1 = ps_bound_k(__shfl(k1, src));
                    const int t_hdr = __shfl(hdr, src), t_range = __shfl(kind == 0 ? r_out : r_in, src);
                    const float4 ref = make_float4(__shfl(kind == 0 ? a_in : a_out, src), __shfl(kind == 0 ? rgb_in[0] : rgb_out[0], src),
                                                   __shfl(kind == 0 ? rgb_in[1] : rgb_out[1], src),
                                                   __shfl(kind == 0 ? rgb_in[2] : rgb_out[2], src));
                    const int t_line = t_hdr & 15;
                    const bool t_use0 = (t_hdr >> 7) & 1, t_use1 = (t_hdr >> 8) & 1;
                    const int from = (t_range & 0xffff) + c * CH, to = min(t_range >> 16, from + CH - 1);
                    const int cnt = mine ? to - from + 1 : 0;
                    const int base = t_line * stride + from;
                    const int rot = (lane - base) & 15;
                    const int t_fn = __shfl(fn, src);
                    if (p.count_terms) {  // ("out" sweeps count every position, long "in" sweeps the face's own pixels)
                        int nt = kind == 0 ? cnt : 0;
                        if (kind == 1)
                            for (int q_ = 0; q_ < cnt; q_++) nt += fimL[base + q_] == t_fn ? 1 : 0;
                        ps_count_terms(nt);
                    }
                    f32x2 ww = {0.0f, 0.0f};
                    // an unused term gets the distance 1 and the weight 0
                    const f32x2 kk = {t_use0 ? t_k0 : 0.0f, t_use1 ? t_k1 : 0.0f};
                    // The records of PG steps are requested together, the next PG while these are worked on (the
                    // compiler keeps the steps of an unrolled loop one behind the other, each waiting for its own LDS
                    // round trip).  No branch in a step: positions behind the chunk's end are read -- LDS, inside the
                    // workgroup's allocation -- and weighted 0.
                    constexpr int PG = 2;  // steps requested together
                    struct Quad { float4 a[PG], g[PG]; int owner[PG], pos[PG]; };
                    auto request = [&](Quad& q, int it0) {
#pragma unroll
                        for (int u = 0; u < PG; u++) {
                            const int pos = (rot + it0 + u) & (CH - 1);
                            q.pos[u] = pos;
                            q.a[u] = recA[base + pos];
                            q.g[u] = recB[base + pos];
                            q.owner[u] = kind == 0 ? 0 : fimL[base + pos];
                        }
                    };
                    if (kind == 0) {
                        // d1 - d1_cross keeps its sign beyond the edge: the +-eps of `dist` is a constant of the sweep.
                        // Both distances of a step at once (packed fp32) and ONE reciprocal for the two,
                        // 1 / (x y) * y and 1 / (x y) * x: v_rcp_f32 is a quarter-rate instruction
                        const float fdir = ((t_hdr >> 6) & 1) ? 1.0f : -1.0f;
                        const f32x2 ee = {t_use0 ? ((0.0f < t_k0 * fdir) ? p.eps : -p.eps) : 1.0f,
                                          t_use1 ? ((0.0f < t_k1 * fdir) ? p.eps : -p.eps) : 1.0f};
                        auto work = [&](const Quad& q) {
#pragma unroll
                            for (int u = 0; u < PG; u++) {
                                float dg = ps_diff_grad(q.a[u], q.g[u], ref);
                                dg = (dg <= 0.0f) ? 0.0f : dg;  // (a NaN stays a NaN, as with upstream's `if (dg <= 0) continue`)
                                dg = q.pos[u] < cnt ? dg : 0.0f;
                                // (the distance of a position behind the chunk's end is taken at the end: beyond it the
                                // sweep may cross the edge, where k * tt + e passes through 0 and 0 * inf would be a NaN)
                                const float tt = (float)(from + min(q.pos[u], cnt - 1)) - t_cross;
                                const f32x2 tt2 = {tt, tt};
                                const f32x2 dist = __builtin_elementwise_fma(kk, tt2, ee);
                                const float r = __builtin_amdgcn_rcpf(dist.x * dist.y);
                                const f32x2 inv = {r * dist.y, r * dist.x};
                                const f32x2 mdg = {-dg, -dg};
                                ww = __builtin_elementwise_fma(mdg, inv, ww);
                            }
                        };
                        Quad x, y;
                        request(x, 0);
#pragma unroll 1
                        for (int it0 = 0; it0 < CH; it0 += 2 * PG) {
                            request(y, it0 + PG);
                            work(x);
                            request(x, it0 + 2 * PG);  // (behind the last step: positions wrap inside the chunk, the values are not used)
                            work(y);
                        }
                    } else {
                        auto work = [&](const Quad& q) {
#pragma unroll
                            for (int u = 0; u < PG; u++) {
                                float dg = ps_diff_grad(q.a[u], q.g[u], ref);
                                dg = (dg <= 0.0f) ? 0.0f : dg;
                                dg = ((q.pos[u] < cnt) & (q.owner[u] == t_fn)) ? dg : 0.0f;
                                const float tt = (float)(from + q.pos[u]) - t_cross;
                                float d0_ = t_k0 * tt, d1_ = t_k1 * tt;
                                const float s0 = (0 < d0_) ? p.eps : -p.eps, s1 = (0 < d1_) ? p.eps : -p.eps;
                                d0_ += s0; d1_ += s1;
                                d0_ = t_use0 ? d0_ : 1.0f;
                                d1_ = t_use1 ? d1_ : 1.0f;
                                const float r = __builtin_amdgcn_rcpf(d0_ * d1_);
                                ww.x = __builtin_fmaf(-dg, r * d1_, ww.x);
                                ww.y = __builtin_fmaf(-dg, r * d0_, ww.y);
                            }
                        };
                        Quad x, y;
                        request(x, 0);
#pragma unroll 1
                        for (int it0 = 0; it0 < CH; it0 += 2 * PG) {
                            request(y, it0 + PG);
                            work(x);
                            request(x, it0 + 2 * PG);  // (behind the last step: positions wrap inside the chunk, the values are not used)
                            work(y);
                        }
                    }
                    // The chunks of an item are CONSECUTIVE tasks (at most 16): their sums are added up over the lanes of the
                    // segment and its first lane adds the total to the item's slot with a plain LDS read-modify-write -- an
                    // item has one segment per round, and the rounds of a wave run one behind the other.  (Round 5: these were
                    // two LDS float atomics per round; ds_add_f32 costs ~12 cycles PER ACTIVE LANE on gfx950 -- 770 cycles for
                    // a full wave whatever the addresses, 30 x a ds_add_u64, profiles/r05_valu_rate_probe.txt -- i.e. as much
                    // as the sixteen terms of the chunks themselves.)
                    float sx = (mine && t_use0) ? ww.x : 0.0f, sy = (mine && t_use1) ? ww.y : 0.0f;
                    const int seg = mine ? src : -1 - lane;
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) {
                        // (every shuffle in full-wave control flow: a lane that is masked off hands out zeros)
                        const float ox = __shfl_down(sx, off), oy = __shfl_down(sy, off);
                        const int os = __shfl_down(seg, off);
                        const bool same = lane + off < MR_WAVE && os == seg;
                        sx += same ? ox : 0.0f;
                        sy += same ? oy : 0.0f;
                    }
                    const int prev = __shfl_up(seg, 1);
                    const bool head = mine && (lane == 0 || prev != seg);
                    if (head && (sx != 0.0f || sy != 0.0f)) {
                        float2 a = acc[src];
                        a.x += sx; a.y += sy;
                        acc[src] = a;
                    }
                }
                __builtin_amdgcn_wave_barrier();  // (the next kind / batch overwrites the task list)
            }
            // an entry's lines -> one pair of sums -> the face's row (zeroed by compact_owners_kernel)
            g0 += acc[lane].x;
            g1 += acc[lane].y;
#pragma unroll
            for (int o = 1; o < L; o <<= 1) {
                g0 += __shfl_xor(g0, o);
                g1 += __shfl_xor(g1, o);
            }
            if (have && loff == 0) {
                if (g0 != 0.0f) unsafeAtomicAdd(&p.grad_faces[i * 9 + 3 * e + comp], g0);
                if (g1 != 0.0f) unsafeAtomicAdd(&p.grad_faces[i * 9 + 3 * (e == 2 ? 0 : e + 1) + comp], g1);
            }
        }
    };

    // The image's front-facing owners, one per thread and round; the records of the first PRE rounds are requested
    // before the strip is staged, so that all of a workgroup's global loads are in flight together.
    constexpr int PRE = 3;
    float4 pre[PRE][2];
#pragma unroll
    for (int j = 0; j < PRE; j++) {
        const unsigned k = (unsigned)(j * PS_T + tid);
        const unsigned kc = k < n_own ? k : 0u;
        pre[j][0] = own_b[2 * kc]; pre[j][1] = own_b[2 * kc + 1];
    }
    stage_strip();
    __syncthreads();
    for (unsigned k0 = 0, j = 0; k0 < n_own; k0 += PS_T, j++) {
        const unsigned k = k0 + tid;
        float4 v01, v2n;
        if (j < PRE) {
#pragma unroll
            for (int jj = 0; jj < PRE; jj++)
                if ((unsigned)jj == j) { v01 = pre[jj][0]; v2n = pre[jj][1]; }
        } else {
            const unsigned kc = k < n_own ? k : 0u;
            v01 = own_b[2 * kc]; v2n = own_b[2 * kc + 1];
        }
        if (k < n_own) {
            const float q[3] = {axis == 0 ? v01.x : v01.y, axis == 0 ? v01.z : v01.w, axis == 0 ? v2n.x : v2n.y};
            unsigned ent[3];
            int n = 0;
#pragma unroll
            for (int e = 0; e < 3; e++) {
                const float q00 = q[e], q10 = q[e == 2 ? 0 : e + 1];
                const int d0_from = (int)fmaxf(ceilf(fminf(q00, q10)), 0.0f);
                const int d0_to = (int)fminf(fmaxf(q00, q10), fis - 1.0f);
                const int lo = max(d0_from, l0), hi = min(d0_to, l0 + L - 1);
                const bool hit = lo <= hi;
                ent[e] = hit ? (k | ((unsigned)e << 24) | ((unsigned)(lo - l0) << 26) | ((unsigned)(hi - lo) << 28)) : 0xffffffffu;
                n += hit ? 1 : 0;
            }
            if (n) {
                unsigned at = atomicAdd(&s_qn, (unsigned)n);
#pragma unroll
                for (int e = 0; e < 3; e++)
                    if (ent[e] != 0xffffffffu) queue[at++] = ent[e];
            }
        }
        __syncthreads();
        const unsigned qn = s_qn;
        if (qn + 3u * PS_T > (unsigned)PS_QCAP || k0 + PS_T >= n_own) {
            if (qn) process(qn);
            __syncthreads();
            if (tid == 0) { s_qn = 0u; s_next = 0u; }
            __syncthreads();
        }
    }
}

template <bool IMG, int L>
__global__ void __launch_bounds__(PS_T) pixel_map_strip_kernel(PixelMapParams p, const unsigned* __restrict__ img_count,
                                                               const float4* __restrict__ img_recs, int strips_axis,
                                                               const unsigned* __restrict__ strip_lists,
                                                               const unsigned* __restrict__ strip_counts, int list_cap) {
    strip_body<IMG, L>(p, img_count, img_recs, strips_axis, strip_lists, strip_counts, list_cap, blockIdx.x);
}

// Kernel D's strips and the E / F gather in ONE launch (round 5).  The two are independent once the owner lists stand -- D adds
// to grad_faces' x / y with atomics, the gather adds its depth terms to the same rows with atomics and writes grad_textures,
// which D never touches -- and they complement each other: the walk is 200+ us of vector arithmetic at three waves per SIMD,
// the gather a latency chain of short workgroups (owner -> face -> probes -> gradients) that waits on memory half of its
// time.  Groups of eight workgroups (one per XCD: the strips' XCD residue is kept) alternate between the two grids while both
// last; a gather workgroup reserves the strips' LDS and registers, which costs it nothing (144 registers: three workgroups
// per compute unit either way).  A first version ran the gather on a second, higher-priority stream (fork / join events):
// 0.375 -> 0.334 ms in a process with two queues, but 0.47 ms inside bench.py's full run -- with the five or more queues that
// process has, every cross-queue dependency waited for a ~50 us scheduling quantum (profiles/r05_def_two_streams_trace.txt).
template <bool IMG, int L, bool TEX, bool DEPTH>
__global__ void __launch_bounds__(PS_T) strip_gather_kernel(PixelMapParams p, const unsigned* __restrict__ img_count,
                                                            const float4* __restrict__ img_recs, int strips_axis,
                                                            const unsigned* __restrict__ strip_lists,
                                                            const unsigned* __restrict__ strip_counts, int list_cap,
                                                            GatherParams g, unsigned gather_groups) {
    const unsigned grp = blockIdx.x >> 3, r = blockIdx.x & 7u;
    // the gather's workgroups first: short, and its few long ones (faces with large boxes) start early
    const bool gather = grp < gather_groups;
    const unsigned vg = gather ? grp : grp - gather_groups;
    if (gather) gather_body<IMG, TEX, DEPTH>(g, vg * 8u + r, gather_groups * 8u);
    else strip_body<IMG, L>(p, img_count, img_recs, strips_axis, strip_lists, strip_counts, list_cap, vg * 8u + r);
}


// backward workspace: per-face "owns a pixel" flags | owner count | per-image counts and line ranges | owner list |
// per-image owner records (the gather needs the flags, the count and the list)
struct OwnerList {
    uint8_t* owns;
    unsigned* counter;
    unsigned* img_count;  // [B] owners per image, then [B][4] their line ranges (behind the counter: one memset clears all)
    uint32_t* list;
    float4* img_recs;     // [B][F][2] the front-facing owners image by image (compact_owners_kernel)
    int64_t clear_bytes;  // flags, counter and counts: what a call clears
    int64_t bytes;
};
static OwnerList owner_list(void* workspace, int B, int F) {
    Carve c;
    OwnerList o;
    o.owns = at_offset<uint8_t>(workspace, c.take((int64_t)B * F));
    o.counter = at_offset<unsigned>(workspace, c.take(256));
    o.img_count = at_offset<unsigned>(workspace, c.take(20LL * B));
    o.clear_bytes = c.total();
    o.list = at_offset<uint32_t>(workspace, c.take((int64_t)B * F * 4));
    o.img_recs = at_offset<float4>(workspace, c.take((int64_t)B * F * 32));
    o.bytes = c.total();
    return o;
}
// flags -> lists (+ zero rows); the workspace's flags and counts must have been cleared (ol.clear_bytes) and marked
static int launch_compact(const CompactPlan& plan, const PixelMapParams& q, const OwnerList& ol, bool per_image, hipStream_t s,
                          unsigned* strip_w = nullptr, int strip_l = 1, int strips_axis = 0) {
    if (plan.status != MR_OK || !plan.launch) return plan.status;
    hipLaunchKernelGGL(compact_owners_kernel, dim3(plan.wgs), dim3(CO_TPB), 0, s, q, (const uint8_t*)ol.owns, ol.counter,
                       ol.list, per_image ? ol.img_count : (unsigned*)nullptr, per_image ? ol.img_recs : (float4*)nullptr, plan.chunks,
                       strip_w, strip_l, strips_axis);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

// ... + kernel D's strip bookkeeping behind it: weights [B][2 strips_axis], per-XCD lists [8][cap], their lengths [8]
struct StripLists {
    unsigned* weights;
    unsigned* lists;
    unsigned* counts;
    int64_t bytes;
};
static StripLists strip_lists(void* workspace, int B, int F, const StripShape& shape) {
    StripLists sl{};
    if (shape.lines == 0) return sl;  // (a raster whose lines do not fit LDS: no strips, no bytes)
    void* base = at_offset<char>(workspace, owner_list(workspace, B, F).bytes);
    Carve c;
    sl.weights = at_offset<unsigned>(base, c.take(shape.n_weights * 4));
    sl.lists = at_offset<unsigned>(base, c.take(8LL * shape.cap * 4));
    sl.counts = at_offset<unsigned>(base, c.take(256));
    sl.bytes = c.total();
    return sl;
}
static int64_t pixel_map_workspace_bytes(int B, int F, int is) {
    return owner_list(nullptr, B, F).bytes + strip_lists(nullptr, B, F, strip_shape(B, is)).bytes;
}

// the marking pass over the face index map (plan_mark); `weights` (nullable): the strip weights it clears on the way
static int launch_mark_owners(const MarkPlan& plan, const int32_t* fim, uint8_t* owns, int F, unsigned* weights, int64_t n_weights,
                              hipStream_t s) {
    if (plan.quads) return launch1d(mark_owners_kernel, plan.threads, s, fim, owns, plan.items, plan.ppi, F, weights, n_weights);
    return launch1d(mark_owners_scalar_kernel, plan.threads, s, fim, owns, plan.items, plan.ppi, F, weights, n_weights);
}

// the strip kernel with the E / F gather inside, for a strip of L lines
template <bool IMG, int L>
static auto strip_gather_for(GatherForm form) {
    switch (form) {
    case GatherForm::TEX_DEPTH: return strip_gather_kernel<IMG, L, true, true>;
    case GatherForm::TEX: return strip_gather_kernel<IMG, L, true, false>;
    default: return strip_gather_kernel<IMG, L, false, true>;
    }
}

// kernel D (plan_pixel_map): by strips, or the plane-reading per-face walk
// `g` (nullable): the E / F gather of the same call, which goes out INSIDE the strip kernel's launch when plan.fused
template <bool IMG>
static int launch_pixel_map(const PixelMapPlan& plan, const PixelMapParams& p, void* workspace, hipStream_t s, const GatherParams* g = nullptr) {
    if (!plan.strips) return launch1d(pixel_map_kernel<IMG>, plan.walk_threads, s, p);
    const OwnerList ol0 = owner_list(workspace, p.B, p.F);
    hipError_t e0 = hipMemsetAsync(ol0.owns, 0, ol0.clear_bytes, s);  // flags and the counts behind them
    if (e0 != hipSuccess) return (int)e0;
    const StripLists sl = strip_lists(workspace, p.B, p.F, plan.shape);
    int rc = launch_mark_owners(plan.mark, p.fim, ol0.owns, p.F, sl.weights, plan.shape.n_weights, s);
    if (rc != MR_OK || !plan.after_mark) return rc;
    PixelMapParams q = p;
    q.zero_owner_rows = 1;
    const int strip_l = plan.shape.lines, strips_axis = plan.shape.strips_axis, cap = plan.shape.cap;
    rc = launch_compact(plan.compact, q, ol0, true, s, sl.weights, strip_l, strips_axis);
    if (rc != MR_OK) return rc;
    hipLaunchKernelGGL(strip_list_kernel, dim3(8), dim3(SL_T), 0, s, (const unsigned*)sl.weights, sl.lists, sl.counts, p.B,
                       plan.shape.strips, cap);
    MR_CHECK_LAUNCH();
    if (plan.status_grid != MR_OK) return plan.status_grid;
    if constexpr (IMG) {  // (only mr_render_backward has a gather to fuse: no raster-orientation instantiations)
    if (plan.fused) {
        auto fused_kernel = strip_l == 4 ? strip_gather_for<IMG, 4>(plan.gather)
                                         : (strip_l == 2 ? strip_gather_for<IMG, 2>(plan.gather) : strip_gather_for<IMG, 1>(plan.gather));
        hipLaunchKernelGGL(fused_kernel, dim3(plan.fused_wgs), dim3(PS_T), plan.lds, s, p, (const unsigned*)ol0.img_count,
                           (const float4*)ol0.img_recs, strips_axis, (const unsigned*)sl.lists, (const unsigned*)sl.counts, cap, *g,
                           plan.gather_groups);
        MR_CHECK_LAUNCH();
        return MR_OK;
    }
    }
    auto kernel = strip_l == 4 ? pixel_map_strip_kernel<IMG, 4> : (strip_l == 2 ? pixel_map_strip_kernel<IMG, 2> : pixel_map_strip_kernel<IMG, 1>);
    hipLaunchKernelGGL(kernel, dim3(plan.wgs), dim3(PS_T), plan.lds, s, p, (const unsigned*)ol0.img_count,
                       (const float4*)ol0.img_recs, strips_axis, (const unsigned*)sl.lists, (const unsigned*)sl.counts, cap);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

}  // namespace mr

using namespace mr;

extern "C" int64_t mr_render_backward_list_workspace_bytes(int batch_size, int num_faces) {
    if (batch_size < 0 || num_faces < 0) return MR_ERR_BADARG;
    return owner_list(nullptr, batch_size, num_faces).bytes;
}

extern "C" int64_t mr_render_backward_workspace_bytes(int batch_size, int num_faces, int image_size) {
    if (batch_size < 0 || num_faces < 0 || image_size <= 0) return MR_ERR_BADARG;
    return pixel_map_workspace_bytes(batch_size, num_faces, image_size);
}

extern "C" int mr_backward_pixel_map(const float* faces, const int32_t* face_index_map,
                                     const float* rgb_map, const float* alpha_map,
                                     const float* grad_rgb_map, const float* grad_alpha_map,
                                     float* grad_faces, int batch_size, int num_faces, int image_size,
                                     float eps, int return_rgb, int return_alpha, mr_stream_t stream) {
    if (!faces || !face_index_map || !grad_faces) return MR_ERR_BADARG;
    if (return_rgb && (!rgb_map || !grad_rgb_map)) return MR_ERR_BADARG;
    if (return_alpha && (!alpha_map || !grad_alpha_map)) return MR_ERR_BADARG;
    if (batch_size < 0 || num_faces < 0 || image_size <= 0) return MR_ERR_BADARG;
    if (!return_rgb && !return_alpha) return MR_OK;
    PixelMapParams p{};  // (value-initialised, then filled: the padding bytes are kernel-argument bytes too)
    p.faces = faces; p.fim = face_index_map; p.rgb = rgb_map; p.alpha = alpha_map; p.grad_rgb = grad_rgb_map; p.grad_alpha = grad_alpha_map;
    p.grad_faces = grad_faces; p.B = batch_size; p.F = num_faces; p.is = image_size; p.eps = eps;
    p.return_rgb = return_rgb; p.return_alpha = return_alpha;
    if (batch_size == 0 || num_faces == 0) return MR_OK;
    // scratch for the walk by strips, stream-ordered like the forward entry point's record list;
    // if it cannot be had the plane-reading kernel does the same job
    hipStream_t s = (hipStream_t)stream;
    void* work = nullptr;
    const int64_t bytes = pixel_map_workspace_bytes(batch_size, num_faces, image_size);
    if (hipMallocAsync(&work, (size_t)bytes, s) != hipSuccess) {
        (void)hipGetLastError();
        work = nullptr;
    }
    const PixelMapPlan plan = plan_pixel_map(batch_size, num_faces, image_size, strips_apply(batch_size, num_faces, image_size, work ? bytes : 0, bytes, 0));
    const int rc = launch_pixel_map<false>(plan, p, work, s);
    if (work) (void)hipFreeAsync(work, s);
    return rc;
}

extern "C" int mr_backward_textures(const int32_t* face_index_map, const float* sampling_weight_map,
                                    const int32_t* sampling_index_map, const float* grad_rgb_map,
                                    float* grad_textures, int batch_size, int num_faces, int image_size,
                                    int texture_size, mr_stream_t stream) {
    if (!face_index_map || !sampling_weight_map || !sampling_index_map || !grad_rgb_map || !grad_textures)
        return MR_ERR_BADARG;
    if (batch_size < 0 || num_faces < 0 || image_size <= 0 || texture_size < 2) return MR_ERR_BADARG;
    const int64_t npx = (int64_t)batch_size * image_size * image_size;
    return launch1d(textures_atomic_stored_kernel, npx, (hipStream_t)stream, face_index_map,
                    sampling_weight_map, sampling_index_map, grad_rgb_map, grad_textures, npx, num_faces,
                    image_size, texture_size);
}

extern "C" int mr_backward_depth_map(const float* faces, const float* depth_map,
                                     const int32_t* face_index_map, const float* face_inv_map,
                                     const float* weight_map, const float* grad_depth_map,
                                     float* grad_faces, int batch_size, int num_faces, int image_size,
                                     mr_stream_t stream) {
    if (!faces || !depth_map || !face_index_map || !face_inv_map || !weight_map || !grad_depth_map ||
        !grad_faces)
        return MR_ERR_BADARG;
    if (batch_size < 0 || num_faces < 0 || image_size <= 0) return MR_ERR_BADARG;
    const int64_t npx = (int64_t)batch_size * image_size * image_size;
    return launch1d(depth_atomic_stored_kernel, npx, (hipStream_t)stream, faces, depth_map, face_index_map,
                    face_inv_map, weight_map, grad_depth_map, grad_faces, npx, num_faces, image_size);
}

// the E / F gather on its own, in a plan's form
static void (*gather_kernel_of(GatherForm form))(GatherParams) {
    switch (form) {
    case GatherForm::TEX_DEPTH: return gather_kernel<true, true, true>;
    case GatherForm::TEX: return gather_kernel<true, true, false>;
    case GatherForm::DEPTH: return gather_kernel<true, false, true>;
    case GatherForm::NONE: break;
    }
    return gather_kernel<true, false, false>;
}

extern "C" int mr_render_backward(const float* faces, const float* textures,
                                  const int32_t* face_index_map, const float* rgb_img,
                                  const float* alpha_img, const float* grad_rgb_img,
                                  const float* grad_alpha_img, const float* grad_depth_img,
                                  float* grad_faces, float* grad_textures, void* workspace,
                                  int64_t workspace_bytes, int batch_size, int num_faces,
                                  int image_size, int texture_size, float near_, float far_, float eps,
                                  int return_rgb, int return_alpha, int return_depth, int flags,
                                  mr_stream_t stream) {
    (void)textures; (void)near_; (void)far_;
    if (batch_size < 0 || num_faces < 0 || image_size <= 0) return MR_ERR_BADARG;
    if (batch_size == 0 || num_faces == 0) return MR_OK;
    if (!faces || !face_index_map) return MR_ERR_BADARG;
    if (grad_textures && (!return_rgb || !grad_rgb_img || texture_size < 2)) return MR_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    // plan
    BackwardRequest req{};
    req.B = batch_size; req.F = num_faces; req.is = image_size; req.ts = texture_size; req.flags = flags; req.eps = eps;
    req.grad_faces = grad_faces != nullptr; req.grad_textures = grad_textures != nullptr;
    req.rgb = return_rgb && grad_rgb_img && rgb_img; req.alpha = return_alpha && grad_alpha_img && alpha_img;
    req.depth = return_depth && grad_depth_img;
    req.workspace_bytes = workspace ? workspace_bytes : 0;
    req.list_bytes = owner_list(nullptr, batch_size, num_faces).bytes;
    req.full_bytes = pixel_map_workspace_bytes(batch_size, num_faces, image_size);
    const BackwardPlan plan = plan_render_backward(req);
    // the E / F gather of the faces that own a pixel (or of all of them without a list)
    GatherParams g{};
    g.faces = faces; g.fim = face_index_map;
    g.grad_rgb = plan.gather_tex ? grad_rgb_img : nullptr;
    g.grad_depth = plan.want_f ? grad_depth_img : nullptr;
    g.grad_faces = grad_faces;
    g.grad_textures = plan.gather_tex ? grad_textures : nullptr;
    g.B = batch_size; g.F = num_faces; g.is = image_size; g.eps = eps;
    g.accumulate_faces = plan.accumulate_faces ? 1 : 0;
    const OwnerList ol = owner_list(workspace, batch_size, num_faces);
    if (plan.use_list) { g.owners = ol.list; g.n_owners = ol.counter; }
    // launch
    int rc = MR_OK;
    if (plan.want_d) {
        PixelMapParams p{};  // (value-initialised, then filled: the padding bytes are kernel-argument bytes too)
        p.faces = faces; p.fim = face_index_map; p.rgb = rgb_img; p.alpha = alpha_img; p.grad_rgb = grad_rgb_img; p.grad_alpha = grad_alpha_img;
        p.grad_faces = grad_faces; p.B = batch_size; p.F = num_faces; p.is = image_size; p.eps = eps;
        p.return_rgb = req.rgb; p.return_alpha = req.alpha; p.write_backfacing = 1; p.count_terms = plan.count_terms ? 1 : 0;
        p.zero_textures = plan.zero_textures_in_d ? grad_textures : nullptr;
        rc = launch_pixel_map<true>(plan.pixel_map, p, workspace, s, &g);
        if (rc != MR_OK) return rc;
    } else if (plan.list_only) {
        hipError_t e = hipMemsetAsync(ol.owns, 0, ol.clear_bytes, s);  // flags and the counts behind them
        if (e != hipSuccess) return (int)e;
        rc = launch_mark_owners(plan.mark, face_index_map, ol.owns, num_faces, nullptr, 0, s);
        if (rc != MR_OK) return rc;
        PixelMapParams q{};
        q.faces = faces; q.grad_faces = grad_faces; q.B = batch_size; q.F = num_faces; q.is = image_size;
        q.write_backfacing = 1;
        q.zero_textures = plan.zero_textures_in_list ? grad_textures : nullptr;
        rc = launch_compact(plan.compact, q, ol, false, s);
        if (rc != MR_OK) return rc;
    }
    if (plan.tex_atomics) {
        hipError_t e = hipMemsetAsync(grad_textures, 0, plan.tex_bytes, s);
        if (e != hipSuccess) return (int)e;
        rc = launch1d(textures_atomic_recompute_kernel<true>, plan.tex_threads, s, faces, face_index_map, grad_rgb_img, grad_textures,
                      plan.tex_threads, num_faces, image_size, texture_size, eps);
        if (rc != MR_OK) return rc;
    }
    if (plan.gather_threads > 0) rc = launch1d(gather_kernel_of(plan.gather_form), plan.gather_threads, s, g);
    return rc;
}

extern "C" int mr_pixel_map_terms(uint64_t* terms_host, int reset) {
    if (!terms_host) return MR_ERR_BADARG;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    unsigned long long v = 0ull;
    e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(mr::mr_pixel_map_terms_counter), sizeof(v), 0, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    *terms_host = (uint64_t)v;
    if (reset) {
        v = 0ull;
        e = hipMemcpyToSymbol(HIP_SYMBOL(mr::mr_pixel_map_terms_counter), &v, sizeof(v), 0, hipMemcpyHostToDevice);
        if (e != hipSuccess) return (int)e;
    }
    return MR_OK;
}
