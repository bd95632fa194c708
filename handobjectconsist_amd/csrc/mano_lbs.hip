// mano_lbs.hip -- MANO linear-blend skinning for gfx950 (MI355X): SURVEY 8a row a19 / 8f "f1".
//
// Replaces manopth's ManoLayer.forward (third-party; called at /root/reference/meshreg/models/
// manobranch.py:130-136; arithmetic as restated in SURVEY appendix B.10) and its autograd:
//   pose PCA -> axis-angle -> rotations (via quaternions) -> pose blend-shape features,
//   v_posed = template + [betas | pose features] x blend shapes            <- the one GEMM-shaped step
//   joints  = J_regressor x (template + shape blend shapes)  (pre-multiplied regressors)
//   kinematic chain of 16 rigid transforms, skinning, joints + finger tips, centring, mm scale.
// Kernels:
//   mano_pre_kernel       one wave per sample: PCA, rotations, joints, chain, corrected transforms
//   mano_blend_kernel     v_posed = coeff[B,K] x blend[K,2334] on the MATRIX CORES: v_mfma_f32_32x32x2_f32
//                         (fp32 in / fp32 accumulate -- bitwise a k-ordered fmaf chain, i.e. what the BLAS
//                         kernel it replaces computes), one 32 x 32 tile per wave
//   mano_skin_kernel      one thread per (sample, vertex): blended 3x4 transform, vertex, finger tips
//   mano_skin_bwd_kernel  per (sample, 256-vertex chunk): d v_posed and the chunk's share of d transforms
//   mano_blend_bwd_kernel d coeff = d v_posed[B,2334] x blend^T on the matrix cores, split-K partials
//   mano_pre_bwd_kernel   one wave per sample: sums the partials, chain / Rodrigues / PCA adjoints
// This is the only GEMM-shaped work on the whole path (M = 2334, K = 145, N = batch).
// One family of kernels serves both entry-point pairs.  What a call adds to plain skinning -- a translation under manopth's
// rule, the ground-truth epilogue -- arrives in ManoFull at run time; the network's call (mr_mano_forward / mr_mano_backward:
// PCA pose, a joint centre or none) passes an empty one, the general call (mr_mano_forward_full / mr_mano_backward_full,
// DESIGN 18) fills it and may take the 48-value axis-angle pose and a finger-tip centre.  The pose form is the only
// template parameter.
#include "mr_common.hpp"

namespace mr {

constexpr int MN_V = 778, MN_J = 16, MN_NV3 = MN_V * 3, MN_KP = 146;  // K = 10 + 135, padded to even
constexpr int MN_TIPS = 5, MN_JT = MN_J + MN_TIPS;
constexpr int MN_SPLITK = 32;  // split-K factor of the backward GEMM

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ManoConst {
    const float* comps;    // [ncomps,45]
    const float* mean;     // [45]
    const float* js;       // [48,10]   J_regressor x shapedirs
    const float* jt;       // [48]      J_regressor x template
    const float* blend;    // [MN_KP, 2334]  k-major: rows 0..9 shapedirs, 10..144 posedirs, 145 zero
    const float* templ;    // [2334]
    const float* weights;  // [778,16]
    const int* parents;    // [16], parents[0] = -1
    const int* tips;       // [5] vertex ids
    const int* reorder;    // [21] output joint k = cat(joints, tips)[reorder[k]]
    int ncomps, center;    // center: index into cat(joints, tips) BEFORE the reorder, or -1; >= 16: a finger tip
};

// what a call adds to plain skinning; all zero (ManoFull{}) = nothing extra, the network's call
struct ManoFull {
    const float* trans;        // [B,3] th_trans, or NULL
    int ntrans;                // 3 B (0 without a translation): the bound of the all-zero scan
    float* tflag;              // [B] workspace: 1.0f where the translation is in force (every sample holds the same value);
                               //   NULL = no translation in force: mano_pre_kernel writes no flag and nobody reads one
    float out_scale;           // the rigid epilogue, applied iff post_rot != NULL: x = v * out_scale; x = x + post_trans[b];
    const float* post_trans;   //   x = post_rot[b] x; x = x - post_trans2[b]   (either translation may be NULL)
    const float* post_rot;     // [B,9]
    const float* post_trans2;  // [B,3]
};
constexpr int MN_POSE_PCA = 0, MN_POSE_AXISANG = 1;  // MR_MANO_POSE_*

__device__ __forceinline__ bool trans_in_force(const ManoFull& mf, int b) { return mf.tflag && mf.tflag[b] != 0.0f; }

// ---------------------------------------------------------------------------------------------------
// small helpers (per-lane serial 3x3 / 3x4 algebra; everything here is a few hundred flops per sample)
// ---------------------------------------------------------------------------------------------------
// 3x4 rigid transforms [R | t], row-major 12 floats: C = A o B
__device__ __forceinline__ void rigid_mul(const float* A, const float* B, float* C) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float v = fmaf(A[4 * r + 2], B[8 + c], fmaf(A[4 * r + 1], B[4 + c], A[4 * r] * B[c]));
            if (c == 3) v += A[4 * r + 3];
            C[4 * r + c] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
// one wave per sample.  Outputs: coeff[B,MN_KP], G[B,16,12] (chain), G2[B,16,12] (rest-pose corrected),
// rots[B,16,9], joints[B,16,3]; tflag[B] where the call has one.
template <int FORM>
__global__ void __launch_bounds__(64) mano_pre_kernel(ManoConst mc, ManoFull mf, const float* __restrict__ pose,
                                                      const float* __restrict__ betas, float* __restrict__ coeff,
                                                      float* __restrict__ G, float* __restrict__ G2,
                                                      float* __restrict__ rots, float* __restrict__ joints,
                                                      float* __restrict__ full_pose_out, int B) {
    __shared__ float s_pose[48], s_R[MN_J * 9], s_J[48], s_G[MN_J * 12];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int np = FORM == MN_POSE_AXISANG ? 48 : 3 + mc.ncomps;
    if (lane < 3) s_pose[lane] = pose[b * np + lane];
    if (lane < 45) {
        if constexpr (FORM == MN_POSE_AXISANG) {
            s_pose[3 + lane] = mc.mean[lane] + pose[b * np + 3 + lane];
        } else {
            float acc = 0.0f;
            for (int c = 0; c < mc.ncomps; c++) acc = fmaf(pose[b * np + 3 + c], mc.comps[c * 45 + lane], acc);
            s_pose[3 + lane] = mc.mean[lane] + acc;
        }
    }
    if (mf.tflag) {
        // manopth's rule: a translation whose norm over the WHOLE tensor is zero counts as absent.  Every sample's wave
        // scans all 3 B values and ORs their magnitude bits: no flag shared between samples, no atomic, no second launch
        unsigned bits = 0u;
        for (int i = lane; i < mf.ntrans; i += 64) bits |= __float_as_uint(mf.trans[i]) & 0x7fffffffu;
        const bool in_force = __ballot(bits != 0u) != 0ull;
        if (lane == 0) mf.tflag[b] = in_force ? 1.0f : 0.0f;
    }
    if (lane < 48) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 10; k++) acc = fmaf(betas[b * 10 + k], mc.js[lane * 10 + k], acc);
        s_J[lane] = acc + mc.jt[lane];
    }
    __syncthreads();
    if (lane < 48) {
        full_pose_out[b * 48 + lane] = s_pose[lane];
        joints[b * 48 + lane] = s_J[lane];
    }
    if (lane < MN_J) {
        float R[9];
        rodrigues(&s_pose[3 * lane], R, nullptr);
#pragma unroll
        for (int k = 0; k < 9; k++) {
            s_R[lane * 9 + k] = R[k];
            rots[(b * MN_J + lane) * 9 + k] = R[k];
            if (lane > 0) coeff[b * MN_KP + 10 + (lane - 1) * 9 + k] = R[k] - ((k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f);
        }
    }
    if (lane < 10) coeff[b * MN_KP + lane] = betas[b * 10 + lane];
    if (lane == 10) coeff[b * MN_KP + MN_KP - 1] = 0.0f;
    __syncthreads();
    if (lane == 0) {  // the chain: 16 rigid products, a few hundred flops
        for (int j = 0; j < MN_J; j++) {
            const int pa = mc.parents[j];
            float rel[12];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) rel[4 * r + c] = s_R[j * 9 + 3 * r + c];
                rel[4 * r + 3] = pa < 0 ? s_J[3 * j + r] : s_J[3 * j + r] - s_J[3 * pa + r];
            }
            if (pa < 0) {
#pragma unroll
                for (int k = 0; k < 12; k++) s_G[j * 12 + k] = rel[k];
            } else {
                rigid_mul(&s_G[pa * 12], rel, &s_G[j * 12]);
            }
        }
    }
    __syncthreads();
    for (int k = lane; k < MN_J * 12; k += 64) {
        const int j = k / 12, e = k % 12, r = e / 4, c = e % 4;
        float v = s_G[k];
        G[b * MN_J * 12 + k] = v;
        if (c == 3)  // t - R J
            v = v - fmaf(s_G[j * 12 + 4 * r + 2], s_J[3 * j + 2],
                         fmaf(s_G[j * 12 + 4 * r + 1], s_J[3 * j + 1], s_G[j * 12 + 4 * r] * s_J[3 * j]));
        G2[b * MN_J * 12 + k] = v;
    }
    // (every row of jtr_out comes from mano_skin_kernel: the centre may be a finger tip, a skinned vertex)
}

// D[M = batch rows, N = 2334] = coeff[B, MN_KP] x blend[MN_KP, 2334] + template; one 32 x 32 tile per wave
__global__ void __launch_bounds__(64) mano_blend_kernel(const float* __restrict__ coeff, const float* __restrict__ blend,
                                                        const float* __restrict__ templ, float* __restrict__ v_posed,
                                                        int B) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
    const int i = lane & 31, kh = lane >> 5;
    const int row = min(m0 + i, B - 1), col = min(n0 + i, MN_NV3 - 1);
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (int k = 0; k < MN_KP; k += 2) {
        const float a = coeff[row * MN_KP + k + kh];        // A[i][k]
        const float bb = blend[(k + kh) * MN_NV3 + col];    // B[k][j]
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
    }
    // C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int n = n0 + i;
    if (n < MN_NV3) {
        const float t = templ[n];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (m < B) v_posed[(int64_t)m * MN_NV3 + n] = acc[r] + t;
        }
    }
}

// blended 3x4 transform of vertex v applied to its posed position
__device__ __forceinline__ void skin_vertex(const float* __restrict__ weights, const float* s_G2,
                                            const float* __restrict__ v_posed, int b, int v, float* o) {
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = 0.0f;
    for (int j = 0; j < MN_J; j++) {
        const float w = weights[v * MN_J + j];
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = fmaf(w, s_G2[j * 12 + e], T[e]);
    }
    const float* vp = v_posed + ((int64_t)b * MN_V + v) * 3;
    const float p[3] = {vp[0], vp[1], vp[2]};
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = fmaf(T[4 * r + 2], p[2], fmaf(T[4 * r + 1], p[1], T[4 * r] * p[0])) + T[4 * r + 3];
}

// translation or centre, the millimetre scale, then the rigid epilogue where there is one -- separate multiplies and adds in
// the order of the host code it stands for (scale, translate, rotate, subtract)
__device__ __forceinline__ void full_finish(const ManoFull& mf, int b, bool in_force, bool centred, const float* off,
                                            float* o) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = (in_force ? o[r] + off[r] : (centred ? o[r] - off[r] : o[r])) * 1000.0f;
    if (mf.post_rot) {
        float x[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            x[r] = o[r] * mf.out_scale;
            if (mf.post_trans) x[r] = x[r] + mf.post_trans[b * 3 + r];
        }
        const float* R = mf.post_rot + b * 9;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            o[r] = R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2];
            if (mf.post_trans2) o[r] = o[r] - mf.post_trans2[b * 3 + r];
        }
    }
}

// one thread per (sample, vertex); block 0 of a sample also writes its 16 joint rows
__global__ void __launch_bounds__(256) mano_skin_kernel(ManoConst mc, ManoFull mf, const float* __restrict__ v_posed,
                                                        const float* __restrict__ G, const float* __restrict__ G2,
                                                        float* __restrict__ verts_out, float* __restrict__ jtr_out,
                                                        int B) {
    __shared__ float s_G2[MN_J * 12];
    __shared__ float s_off[3];
    const int b = blockIdx.y, v = blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = threadIdx.x; k < MN_J * 12; k += blockDim.x) s_G2[k] = G2[b * MN_J * 12 + k];
    __syncthreads();
    const bool in_force = trans_in_force(mf, b);
    if (threadIdx.x == 0) {  // what every output of the sample is shifted by: the translation, or the centre
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (in_force) {
#pragma unroll
            for (int r = 0; r < 3; r++) c[r] = mf.trans[b * 3 + r];
        } else if (mc.center >= MN_J) {  // a finger tip is a skinned vertex: recomputed here, the same arithmetic
            skin_vertex(mc.weights, s_G2, v_posed, b, mc.tips[mc.center - MN_J], c);
        } else if (mc.center >= 0) {
#pragma unroll
            for (int r = 0; r < 3; r++) c[r] = G[(b * MN_J + mc.center) * 12 + 4 * r + 3];
        }
#pragma unroll
        for (int r = 0; r < 3; r++) s_off[r] = c[r];
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < MN_JT) {  // the joint rows
        const int k = threadIdx.x, src = mc.reorder[k];
        if (src < MN_J) {
            float o[3];
#pragma unroll
            for (int r = 0; r < 3; r++) o[r] = G[(b * MN_J + src) * 12 + 4 * r + 3];
            full_finish(mf, b, in_force, mc.center >= 0, s_off, o);
#pragma unroll
            for (int r = 0; r < 3; r++) jtr_out[(b * MN_JT + k) * 3 + r] = o[r];
        }
    }
    if (v >= MN_V) return;
    float o[3];
    skin_vertex(mc.weights, s_G2, v_posed, b, v, o);
    full_finish(mf, b, in_force, mc.center >= 0, s_off, o);
#pragma unroll
    for (int r = 0; r < 3; r++) verts_out[((int64_t)b * MN_V + v) * 3 + r] = o[r];
#pragma unroll
    for (int tpi = 0; tpi < MN_TIPS; tpi++)
        if (mc.tips[tpi] == v) {
            for (int k = 0; k < MN_JT; k++)
                if (mc.reorder[k] == MN_J + tpi)
#pragma unroll
                    for (int r = 0; r < 3; r++) jtr_out[(b * MN_JT + k) * 3 + r] = o[r];
        }
}

// ---------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------
// per (sample, chunk of 256 vertices): gradient of v_posed, and the chunk's share of dG2[16,12] and of the
// gradient of the centre (3), written to part[b][chunk][16 * 12 + 3]
constexpr int MN_CHUNKS = (MN_V + 255) / 256;
constexpr int MN_PART = MN_J * 12 + 3;

__global__ void __launch_bounds__(256) mano_skin_bwd_kernel(ManoConst mc, ManoFull mf, const float* __restrict__ v_posed,
                                                            const float* __restrict__ G2,
                                                            const float* __restrict__ grad_verts,
                                                            const float* __restrict__ grad_jtr,
                                                            float* __restrict__ grad_vp, float* __restrict__ part,
                                                            int B) {
    __shared__ float s_G2[MN_J * 12];
    __shared__ float s_gt[256][13];   // g (x) [vp, 1] per vertex of the chunk (12) -- padded
    __shared__ float s_w[256][MN_J + 1];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, v = chunk * 256 + tid;
    for (int k = tid; k < MN_J * 12; k += 256) s_G2[k] = G2[b * MN_J * 12 + k];
    __syncthreads();
    // A finger-tip centre in force: the centre IS vertex cv, so its adjoint -- minus the sum of every incoming
    // gradient of the sample, 778 vertex rows + 21 joint rows -- joins that vertex's gradient.  Summed by the one chunk
    // that holds cv, in a fixed order (strided partial sums, then a tree over LDS): deterministic
    int cv = -1;
    float gctr[3] = {0.0f, 0.0f, 0.0f};
    if (mc.center >= MN_J && !trans_in_force(mf, b)) cv = mc.tips[mc.center - MN_J];
    if (cv >= 0 && cv / 256 == chunk) {  // (uniform over the block)
        float a[3] = {0.0f, 0.0f, 0.0f};
        for (int i = tid; i < MN_V + MN_JT; i += 256) {
            const float* src = i < MN_V ? (grad_verts ? grad_verts + ((int64_t)b * MN_V + i) * 3 : nullptr)
                                        : (grad_jtr ? grad_jtr + (b * MN_JT + (i - MN_V)) * 3 : nullptr);
            if (src)
#pragma unroll
                for (int r = 0; r < 3; r++) a[r] += src[r] * 1000.0f;
        }
#pragma unroll
        for (int r = 0; r < 3; r++) s_gt[tid][r] = a[r];
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h)
#pragma unroll
                for (int r = 0; r < 3; r++) s_gt[tid][r] += s_gt[tid + h][r];
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 3; r++) gctr[r] = -s_gt[0][r];
        __syncthreads();
    }
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (v < MN_V) {
        float T[12], w[MN_J];
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = 0.0f;
        for (int j = 0; j < MN_J; j++) {
            w[j] = mc.weights[v * MN_J + j];
            s_w[tid][j] = w[j];
#pragma unroll
            for (int e = 0; e < 12; e++) T[e] = fmaf(w[j], s_G2[j * 12 + e], T[e]);
        }
#pragma unroll
        for (int r = 0; r < 3; r++) g[r] = grad_verts ? grad_verts[((int64_t)b * MN_V + v) * 3 + r] * 1000.0f : 0.0f;
        if (grad_jtr)
            for (int tpi = 0; tpi < MN_TIPS; tpi++)
                if (mc.tips[tpi] == v)
                    for (int k = 0; k < MN_JT; k++)
                        if (mc.reorder[k] == MN_J + tpi)
#pragma unroll
                            for (int r = 0; r < 3; r++) g[r] += grad_jtr[(b * MN_JT + k) * 3 + r] * 1000.0f;
        if (v == cv)
#pragma unroll
            for (int r = 0; r < 3; r++) g[r] += gctr[r];
        const float* vp = v_posed + ((int64_t)b * MN_V + v) * 3;
        const float p[4] = {vp[0], vp[1], vp[2], 1.0f};
#pragma unroll
        for (int c = 0; c < 3; c++)
            grad_vp[((int64_t)b * MN_V + v) * 3 + c] = fmaf(T[8 + c], g[2], fmaf(T[4 + c], g[1], T[c] * g[0]));
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) s_gt[tid][4 * r + c] = g[r] * p[c];
    } else {
#pragma unroll
        for (int e = 0; e < 12; e++) s_gt[tid][e] = 0.0f;
        for (int j = 0; j < MN_J; j++) s_w[tid][j] = 0.0f;
    }
    s_gt[tid][12] = 0.0f;
    __syncthreads();
    // dG2[j][e] = sum_v w[v][j] * gT[v][e] : one thread per (j, e), fixed order -> deterministic
    if (tid < MN_J * 12) {
        const int j = tid / 12, e = tid % 12;
        float acc = 0.0f;
        for (int u = 0; u < 256; u++) acc = fmaf(s_w[u][j], s_gt[u][e], acc);
        part[((int64_t)b * MN_CHUNKS + chunk) * MN_PART + tid] = acc;
    } else if (tid < MN_J * 12 + 3) {
        // d centre = - sum of the vertex gradients (each vertex subtracts the centre); g = gT[.][4 r + 3]
        // (256 terms one after the other: in double, or the sum -- it is grad trans -- is several fp32 ulps off)
        const int r = tid - MN_J * 12;
        double acc = 0.0;
        for (int u = 0; u < 256; u++) acc += (double)s_gt[u][4 * r + 3];
        part[((int64_t)b * MN_CHUNKS + chunk) * MN_PART + tid] = (float)-acc;
    }
}

// grad_coeff partial[s][B, 160] = grad_vp[B, 2334 (slice s)] x blend^T: split-K on the matrix cores
__global__ void __launch_bounds__(64) mano_blend_bwd_kernel(const float* __restrict__ grad_vp,
                                                            const float* __restrict__ blend,
                                                            float* __restrict__ partial, int B, int Mpad) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32, s = blockIdx.z;
    const int i = lane & 31, kh = lane >> 5;
    const int row = min(m0 + i, B - 1), col = min(n0 + i, MN_KP - 1);
    const int kper = ((MN_NV3 + MN_SPLITK - 1) / MN_SPLITK + 1) & ~1;  // even slice length
    const int k0 = s * kper, k1 = min(k0 + kper, MN_NV3);
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = k0; k < k1; k += 2) {
        const int kk = k + kh;
        const bool in = kk < k1;
        const float a = in ? grad_vp[(int64_t)row * MN_NV3 + kk] : 0.0f;   // A[i][k]
        const float bb = in ? blend[col * MN_NV3 + kk] : 0.0f;            // B[k][j] = blend[j][k]
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
    }
    const int n = n0 + i;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (m < Mpad && n < 160) partial[((int64_t)s * Mpad + m) * 160 + n] = acc[r];
    }
}

// one wave per sample
template <int FORM>
__global__ void __launch_bounds__(64) mano_pre_bwd_kernel(ManoConst mc, ManoFull mf, float* __restrict__ grad_trans,
                                                          const float* __restrict__ full_pose,
                                                          const float* __restrict__ rots,
                                                          const float* __restrict__ joints, const float* __restrict__ G,
                                                          const float* __restrict__ part,
                                                          const float* __restrict__ partial,
                                                          const float* __restrict__ grad_jtr,
                                                          float* __restrict__ grad_pose, float* __restrict__ grad_betas,
                                                          int B, int Mpad) {
    // The adjoints of this kernel are accumulated in DOUBLE: a few thousand flops per sample on one wave, and sums whose
    // terms cancel (a joint's position enters its own transform and every descendant's with opposite signs), so that fp32
    // accumulation left grad betas 5 to 11 fp32 ulps off where the inputs allow 1 to 2 (tests/test_gpu_mano_grads.py).
    // What the forward pass stored (G, rots, joints) and what goes out stay fp32
    __shared__ double s_gG2[MN_J * 12], s_gc[3], s_gcoef[MN_KP], s_gG[MN_J * 12], s_gRd[MN_J * 9], s_gJ[48], s_gt[MN_J][3];
    __shared__ float s_gR[MN_J * 9], s_gp[48];
    __shared__ float s_G[MN_J * 12], s_R[MN_J * 9], s_J[48];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int np = FORM == MN_POSE_AXISANG ? 48 : 3 + mc.ncomps;
    for (int k = lane; k < MN_J * 12; k += 64) {
        double acc = 0.0;
        for (int c = 0; c < MN_CHUNKS; c++) acc += (double)part[((int64_t)b * MN_CHUNKS + c) * MN_PART + k];
        s_gG2[k] = acc;
        s_G[k] = G[b * MN_J * 12 + k];
    }
    if (lane < 3) {
        double acc = 0.0;
        for (int c = 0; c < MN_CHUNKS; c++) acc += (double)part[((int64_t)b * MN_CHUNKS + c) * MN_PART + MN_J * 12 + lane];
        s_gc[lane] = acc;
    }
    for (int k = lane; k < MN_KP; k += 64) {
        double acc = 0.0;
        for (int s = 0; s < MN_SPLITK; s++) acc += (double)partial[((int64_t)s * Mpad + b) * 160 + k];
        s_gcoef[k] = acc;
    }
    for (int k = lane; k < MN_J * 9; k += 64) s_R[k] = rots[b * MN_J * 9 + k];
    if (lane < 48) { s_J[lane] = joints[b * 48 + lane]; s_gJ[lane] = 0.0; }
    __syncthreads();
    // joint rows of jtr: (G[src].t - centre) * 1000 ; centre gradient gathers everything that was centred
    if (lane == 0) {
        double (*gt)[3] = s_gt;  // (indexed by the reorder table: in LDS, not in scratch)
        for (int j = 0; j < MN_J; j++) gt[j][0] = gt[j][1] = gt[j][2] = 0.0;
        double gc[3] = {s_gc[0], s_gc[1], s_gc[2]};
        if (grad_jtr)
            for (int k = 0; k < MN_JT; k++) {
                const int src = mc.reorder[k];
                for (int r = 0; r < 3; r++) {
                    const double g = (double)grad_jtr[(b * MN_JT + k) * 3 + r] * 1000.0;
                    if (src < MN_J) { gt[src][r] += g; gc[r] -= g; }
                    // (tips: their share of the centre gradient is in part[] through the vertex rows)
                }
            }
        // A translation in force: verts = (skinned + trans) * 1000, joints likewise, so d trans = the sum of every incoming
        // gradient x 1000 = -gc, and nothing was centred.  Otherwise a joint centre's adjoint, gc, goes to its joint; a tip
        // centre's went into its vertex (mano_skin_bwd_kernel), part[]'s sum then holds that vertex's addend too and is not
        // used.  (0 - gc, not -gc: the same value for every gc but zero, where all-zero incoming gradients then give +0
        // like every other gradient, not -0)
        const bool in_force = trans_in_force(mf, b);
        if (grad_trans)
            for (int r = 0; r < 3; r++) grad_trans[b * 3 + r] = in_force ? (float)(0.0 - gc[r]) : 0.0f;
        if (mc.center >= 0 && mc.center < MN_J && !in_force)
            for (int r = 0; r < 3; r++) gt[mc.center][r] += gc[r];
        // G2 = [G.R | G.t - G.R J]  ->  dG.R = dG2.R - dG2.t (x) J ; dG.t = dG2.t ; dJ = - G.R^T dG2.t
        for (int j = 0; j < MN_J; j++) {
            for (int r = 0; r < 3; r++) {
                const double gt2 = s_gG2[j * 12 + 4 * r + 3];
                for (int c = 0; c < 3; c++) {
                    s_gG[j * 12 + 4 * r + c] = s_gG2[j * 12 + 4 * r + c] - gt2 * (double)s_J[3 * j + c];
                    s_gJ[3 * j + c] -= (double)s_G[j * 12 + 4 * r + c] * gt2;
                }
                s_gG[j * 12 + 4 * r + 3] = gt2 + gt[j][r];
            }
        }
        // chain, children before parents: G_j = G_p o rel_j, rel_j = [R_j | J_j - J_p]
        for (int j = MN_J - 1; j >= 0; j--) {
            const int pa = mc.parents[j];
            if (pa < 0) {
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) s_gRd[j * 9 + 3 * r + c] = s_gG[j * 12 + 4 * r + c];
                    s_gJ[3 * j + r] += s_gG[j * 12 + 4 * r + 3];
                }
                continue;
            }
            double rel[12];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) rel[4 * r + c] = (double)s_R[j * 9 + 3 * r + c];
                rel[4 * r + 3] = (double)s_J[3 * j + r] - (double)s_J[3 * pa + r];
            }
            // d rel = G_p.R^T dG_j ; d G_p.R += dG_j.R rel.R^T + dG_j.t (x) rel.t ; d G_p.t += dG_j.t
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) {
                    double acc = 0.0;
                    for (int k = 0; k < 3; k++) acc += (double)s_G[pa * 12 + 4 * k + r] * s_gG[j * 12 + 4 * k + c];
                    if (c < 3) s_gRd[j * 9 + 3 * r + c] = acc;
                    else { s_gJ[3 * j + r] += acc; s_gJ[3 * pa + r] -= acc; }
                }
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) {
                    double acc = 0.0;
                    for (int k = 0; k < 4; k++) acc += s_gG[j * 12 + 4 * r + k] * rel[4 * c + k];
                    s_gG[pa * 12 + 4 * r + c] += acc;
                }
                s_gG[pa * 12 + 4 * r + 3] += s_gG[j * 12 + 4 * r + 3];
            }
        }
    }
    __syncthreads();
    // pose features: coeff[10 + 9 (j - 1) + k] = R_j[k] - I
    for (int k = lane; k < MN_J * 9; k += 64) s_gR[k] = (float)(k >= 9 ? s_gRd[k] + s_gcoef[10 + (k - 9)] : s_gRd[k]);
    __syncthreads();
    if (lane < MN_J) {
        float gr[3];
        rodrigues_bwd(&full_pose[b * 48 + 3 * lane], &s_gR[lane * 9], gr);
#pragma unroll
        for (int k = 0; k < 3; k++) s_gp[3 * lane + k] = gr[k];
    }
    __syncthreads();
    if (lane < 3) grad_pose[b * np + lane] = s_gp[lane];
    if constexpr (FORM == MN_POSE_AXISANG) {
        if (lane < 45) grad_pose[b * np + 3 + lane] = s_gp[3 + lane];
    } else if (lane < mc.ncomps) {
        float acc = 0.0f;
        for (int l = 0; l < 45; l++) acc = fmaf(mc.comps[lane * 45 + l], s_gp[3 + l], acc);
        grad_pose[b * np + 3 + lane] = acc;
    }
    if (lane < 10) {
        double acc = s_gcoef[lane];
        for (int l = 0; l < 48; l++) acc += (double)mc.js[l * 10 + lane] * s_gJ[l];
        grad_betas[b * 10 + lane] = (float)acc;
    }
}

}  // namespace mr

using namespace mr;

static ManoConst mano_const(const float* comps, const float* mean, const float* js, const float* jt, const float* blend,
                            const float* templ, const float* weights, const int32_t* parents, const int32_t* tips,
                            const int32_t* reorder, int ncomps, int center) {
    return ManoConst{comps, mean, js, jt, blend, templ, weights, (const int*)parents, (const int*)tips, (const int*)reorder,
                     ncomps, center};
}

// coeff | G | G2 | rots | joints | full_pose | v_posed | grad_vp | part | partial | tflag: float arrays, packed.  Both
// entry-point pairs carve the same regions; tflag lies behind the others, and only mr_mano_full_workspace_floats counts it:
// the network's call has no translation and passes the kernels no flag
struct ManoWork {
    float *coeff, *G, *G2, *rots, *joints, *full_pose, *v_posed, *grad_vp, *part, *partial, *tflag;
    int Mpad;
    int64_t floats, full_floats;  // without / with tflag
};
static ManoWork mano_work(float* w, int64_t B) {
    ManoWork m;
    m.Mpad = (int)((B + 31) / 32 * 32);
    Carve c;
    auto take = [&](int64_t floats) { return at_offset<float>(w, c.take(floats * 4, 4)); };
    m.coeff = take(B * MN_KP); m.G = take(B * MN_J * 12); m.G2 = take(B * MN_J * 12); m.rots = take(B * MN_J * 9);
    m.joints = take(B * 48); m.full_pose = take(B * 48); m.v_posed = take(B * MN_NV3); m.grad_vp = take(B * MN_NV3);
    m.part = take(B * MN_CHUNKS * MN_PART); m.partial = take((int64_t)MN_SPLITK * m.Mpad * 160);
    m.floats = c.total() / 4;
    m.tflag = take(B);
    m.full_floats = c.total() / 4;
    return m;
}

// The three forward launches of either entry point, arguments already checked.  The switch on the pose form is here and in
// mano_launch_backward, nowhere else
static int mano_launch_forward(const ManoConst& mc, const ManoFull& mf, int pose_form, float* workspace, const float* pose,
                               const float* betas, float* verts_out, float* jtr_out, int B, hipStream_t s) {
    const ManoWork m = mano_work(workspace, B);
    const auto pre = pose_form == MN_POSE_AXISANG ? mano_pre_kernel<MN_POSE_AXISANG> : mano_pre_kernel<MN_POSE_PCA>;
    hipLaunchKernelGGL(pre, dim3((unsigned)B), dim3(64), 0, s, mc, mf, pose, betas, m.coeff, m.G, m.G2, m.rots, m.joints,
                       m.full_pose, B);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mano_blend_kernel, dim3((MN_NV3 + 31) / 32, (unsigned)((B + 31) / 32)), dim3(64), 0, s,
                       (const float*)m.coeff, mc.blend, mc.templ, m.v_posed, B);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mano_skin_kernel, dim3(blocks1d(MN_V), (unsigned)B), dim3(256), 0, s, mc, mf, (const float*)m.v_posed,
                       (const float*)m.G, (const float*)m.G2, verts_out, jtr_out, B);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

// ... and the three backward launches; mf.tflag is what the forward call left in the workspace, or NULL
static int mano_launch_backward(const ManoConst& mc, const ManoFull& mf, int pose_form, float* workspace,
                                const float* grad_verts, const float* grad_jtr, float* grad_pose, float* grad_betas,
                                float* grad_trans, int B, hipStream_t s) {
    const ManoWork m = mano_work(workspace, B);
    hipLaunchKernelGGL(mano_skin_bwd_kernel, dim3(MN_CHUNKS, (unsigned)B), dim3(256), 0, s, mc, mf, (const float*)m.v_posed,
                       (const float*)m.G2, grad_verts, grad_jtr, m.grad_vp, m.part, B);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mano_blend_bwd_kernel, dim3(5, (unsigned)(m.Mpad / 32), MN_SPLITK), dim3(64), 0, s,
                       (const float*)m.grad_vp, mc.blend, m.partial, B, m.Mpad);
    MR_CHECK_LAUNCH();
    const auto pre_bwd = pose_form == MN_POSE_AXISANG ? mano_pre_bwd_kernel<MN_POSE_AXISANG> : mano_pre_bwd_kernel<MN_POSE_PCA>;
    hipLaunchKernelGGL(pre_bwd, dim3((unsigned)B), dim3(64), 0, s, mc, mf, grad_trans, (const float*)m.full_pose,
                       (const float*)m.rots, (const float*)m.joints, (const float*)m.G, (const float*)m.part,
                       (const float*)m.partial, grad_jtr, grad_pose, grad_betas, B, m.Mpad);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

// ---------------------------------------------------------------------------------------------------
// the network's call: PCA pose, a joint centre or none, nothing extra (an empty ManoFull, a workspace without tflag)
// ---------------------------------------------------------------------------------------------------
extern "C" int64_t mr_mano_workspace_floats(int batch_size) {
    if (batch_size < 0) return MR_ERR_BADARG;
    return mano_work(nullptr, batch_size).floats;
}

extern "C" int mr_mano_forward(const float* pose_coeffs, const float* betas, const float* comps, const float* hands_mean,
                               const float* js, const float* jt, const float* blend, const float* v_template,
                               const float* weights, const int32_t* parents, const int32_t* tips, const int32_t* reorder,
                               int ncomps, int center, float* workspace, float* verts_out, float* jtr_out,
                               int batch_size, mr_stream_t stream) {
    if (batch_size < 0 || ncomps < 0 || ncomps > 45 || center >= MN_J) return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    if (!pose_coeffs || !betas || !comps || !hands_mean || !js || !jt || !blend || !v_template || !weights || !parents ||
        !tips || !reorder || !workspace || !verts_out || !jtr_out)
        return MR_ERR_BADARG;
    if (batch_size > 65535) return MR_ERR_BADARG;
    const ManoConst mc = mano_const(comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, ncomps,
                                    center);
    return mano_launch_forward(mc, ManoFull{}, MN_POSE_PCA, workspace, pose_coeffs, betas, verts_out, jtr_out, batch_size,
                               (hipStream_t)stream);
}

extern "C" int mr_mano_backward(const float* comps, const float* hands_mean, const float* js, const float* jt,
                                const float* blend, const float* v_template, const float* weights,
                                const int32_t* parents, const int32_t* tips, const int32_t* reorder, int ncomps,
                                int center, float* workspace, const float* grad_verts, const float* grad_jtr,
                                float* grad_pose_coeffs, float* grad_betas, int batch_size, mr_stream_t stream) {
    if (batch_size < 0 || ncomps < 0 || ncomps > 45 || center >= MN_J) return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    if (!comps || !hands_mean || !js || !jt || !blend || !v_template || !weights || !parents || !tips || !reorder ||
        !workspace || !grad_pose_coeffs || !grad_betas)
        return MR_ERR_BADARG;
    if (batch_size > 65535) return MR_ERR_BADARG;
    const ManoConst mc = mano_const(comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, ncomps,
                                    center);
    return mano_launch_backward(mc, ManoFull{}, MN_POSE_PCA, workspace, grad_verts, grad_jtr, grad_pose_coeffs, grad_betas,
                                nullptr, batch_size, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------
// the general call: either pose form, any centre, th_trans, the ground-truth epilogue
// ---------------------------------------------------------------------------------------------------
extern "C" int64_t mr_mano_full_workspace_floats(int batch_size) {
    if (batch_size < 0) return MR_ERR_BADARG;
    return mano_work(nullptr, batch_size).full_floats;
}

// what both general entry points check before anything touches HIP
static int mano_full_check(const float* comps, const float* hands_mean, const float* js, const float* jt, const float* blend,
                           const float* v_template, const float* weights, const int32_t* parents, const int32_t* tips,
                           const int32_t* reorder, int pose_form, int ncomps, int center, const float* workspace,
                           int batch_size) {
    if (pose_form != MN_POSE_PCA && pose_form != MN_POSE_AXISANG) return MR_ERR_BADARG;
    if (ncomps < 1 || ncomps > 45 || center < -1 || center >= MN_JT || batch_size > 65535) return MR_ERR_BADARG;
    if ((pose_form == MN_POSE_PCA && !comps) || !hands_mean || !js || !jt || !blend || !v_template || !weights || !parents ||
        !tips || !reorder || !workspace)
        return MR_ERR_BADARG;
    if (misaligned({comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, workspace}, 3))
        return MR_ERR_BADARG;
    return MR_OK;
}

extern "C" int mr_mano_forward_full(const float* pose, const float* betas, const float* trans, const float* comps,
                                    const float* hands_mean, const float* js, const float* jt, const float* blend,
                                    const float* v_template, const float* weights, const int32_t* parents,
                                    const int32_t* tips, const int32_t* reorder, int pose_form, int ncomps, int center,
                                    float out_scale, const float* post_trans, const float* post_rot,
                                    const float* post_trans2, float* workspace, float* verts_out, float* jtr_out,
                                    int batch_size, mr_stream_t stream) {
    if (batch_size < 0) return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    const int rc = mano_full_check(comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, pose_form,
                                   ncomps, center, workspace, batch_size);
    if (rc != MR_OK) return rc;
    if (!pose || !betas || !verts_out || !jtr_out || (!post_rot && (post_trans || post_trans2))) return MR_ERR_BADARG;
    if (misaligned({pose, betas, trans, post_trans, post_rot, post_trans2, verts_out, jtr_out}, 3)) return MR_ERR_BADARG;
    const ManoConst mc = mano_const(comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, ncomps,
                                    center);
    ManoFull mf{};  // (value-initialised, then filled: its padding bytes are kernel-argument bytes)
    mf.trans = trans; mf.ntrans = trans ? 3 * batch_size : 0; mf.tflag = mano_work(workspace, batch_size).tflag;
    mf.out_scale = out_scale; mf.post_trans = post_trans; mf.post_rot = post_rot; mf.post_trans2 = post_trans2;
    return mano_launch_forward(mc, mf, pose_form, workspace, pose, betas, verts_out, jtr_out, batch_size,
                               (hipStream_t)stream);
}

extern "C" int mr_mano_backward_full(const float* comps, const float* hands_mean, const float* js, const float* jt,
                                     const float* blend, const float* v_template, const float* weights,
                                     const int32_t* parents, const int32_t* tips, const int32_t* reorder, int pose_form,
                                     int ncomps, int center, float* workspace, const float* grad_verts,
                                     const float* grad_jtr, float* grad_pose, float* grad_betas, float* grad_trans,
                                     int batch_size, mr_stream_t stream) {
    if (batch_size < 0) return MR_ERR_BADARG;
    if (batch_size == 0) return MR_OK;
    const int rc = mano_full_check(comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, pose_form,
                                   ncomps, center, workspace, batch_size);
    if (rc != MR_OK) return rc;
    if (!grad_pose || !grad_betas) return MR_ERR_BADARG;
    if (misaligned({grad_verts, grad_jtr, grad_pose, grad_betas, grad_trans}, 3)) return MR_ERR_BADARG;
    const ManoConst mc = mano_const(comps, hands_mean, js, jt, blend, v_template, weights, parents, tips, reorder, ncomps,
                                    center);
    ManoFull mf{};
    mf.tflag = mano_work(workspace, batch_size).tflag; mf.out_scale = 1.0f;
    return mano_launch_backward(mc, mf, pose_form, workspace, grad_verts, grad_jtr, grad_pose, grad_betas, grad_trans,
                                batch_size, (hipStream_t)stream);
}
