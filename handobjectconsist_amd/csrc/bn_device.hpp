// bn_device.hpp -- the device and host layer shared by the trunk's glue kernels (frozen_bn.hip: bn_act, bn_add_bn_act;
// stem_pool.hip: stem_pool in layouts 0, 1, 2).  Every mechanism those kernels have in common is defined here once,
// with its contract next to it.  CONTRACT marks what fixes result bits (expression shapes under -ffp-contract=off,
// summation orders, grid sizes); everything else is plumbing and free to change.
#pragma once
#include <initializer_list>

#include "mr_common.hpp"

namespace mr {

// ---- activation I/O --------------------------------------------------------------------------------------------
// Activations are fp32, or bf16 (the trunk under bf16 autocast) widened on load and rounded to nearest-even on store
// (mr_common.hpp's conversions); all arithmetic is fp32.  T is float or bf16_t, `o` counts elements.
__device__ __forceinline__ float act_to_f32(float v) { return v; }
__device__ __forceinline__ float act_to_f32(bf16_t v) { return bf16_to_f32(v); }
template <typename T> __device__ __forceinline__ T act_from_f32(float v);
template <> __device__ __forceinline__ float act_from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t act_from_f32<bf16_t>(float v) { return f32_to_bf16(v); }

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<bf16_t> { typedef ushort4 type; };

template <typename T>
__device__ __forceinline__ float load1(const void* base, int64_t o) { return act_to_f32(static_cast<const T*>(base)[o]); }
template <typename T>
__device__ __forceinline__ void store1(void* base, int64_t o, float v) { static_cast<T*>(base)[o] = act_from_f32<T>(v); }
// one 16-byte (fp32) / 8-byte (bf16) access: base + o must be aligned to it (the host checks with aligned4)
template <typename T>
__device__ __forceinline__ void load4(const void* base, int64_t o, float* v) {
    const typename Vec4<T>::type t = *reinterpret_cast<const typename Vec4<T>::type*>(static_cast<const T*>(base) + o);
    v[0] = act_to_f32(t.x); v[1] = act_to_f32(t.y); v[2] = act_to_f32(t.z); v[3] = act_to_f32(t.w);
}
template <typename T>
__device__ __forceinline__ void store4(void* base, int64_t o, const float* v) {
    typename Vec4<T>::type t;
    t.x = act_from_f32<T>(v[0]); t.y = act_from_f32<T>(v[1]); t.z = act_from_f32<T>(v[2]); t.w = act_from_f32<T>(v[3]);
    *reinterpret_cast<typename Vec4<T>::type*>(static_cast<T*>(base) + o) = t;
}

// Two-gradient load: an activation with two consumers gets two gradients, summed here instead of by an add pass.
// CONTRACT: g = grad_y, then g += grad_y2 when it is present -- in fp32, after widening.
template <typename T>
__device__ __forceinline__ float load1_grad(const void* grad_y, const void* grad_y2, int64_t o) {
    float g = load1<T>(grad_y, o);
    if (grad_y2) g += load1<T>(grad_y2, o);
    return g;
}
template <typename T>
__device__ __forceinline__ void load4_grad(const void* grad_y, const void* grad_y2, int64_t o, float* g) {
    load4<T>(grad_y, o, g);
    if (grad_y2) {
        float g2[4];
        load4<T>(grad_y2, o, g2);
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] += g2[i];
    }
}

// ReLU that propagates NaN like torch.relu (fmaxf(NaN, 0) would return 0 and hide a diverged trunk from the
// "Loss became nan!" guard)
__device__ __forceinline__ float relu_nan(float z) { return z > 0.0f ? z : (z != z ? z : 0.0f); }

// ---- channel constants -------------------------------------------------------------------------------------------
// A BatchNorm with frozen statistics: z = (x - mean) * a + b per channel.
struct BnAffine {
    const float* weight;  // [C]
    const float* bias;
    const float* mean;
    const float* var;
    float eps;
};
// (value-initialised, then filled: the four bytes behind eps are kernel-argument bytes of every block that holds one)
static inline BnAffine bn_affine(const float* weight, const float* bias, const float* mean, const float* var, float eps) {
    BnAffine f{};
    f.weight = weight; f.bias = bias; f.mean = mean; f.var = var; f.eps = eps;
    return f;
}
// CONTRACT: invstd = 1.0f / sqrtf(var + eps) and a = weight * invstd, exactly these operations; the kernels then form
// d = x - mean and z = d * a + b.  The finish kernel multiplies by the same invstd expression.
__device__ __forceinline__ float bn_invstd(const float* var, float eps, int c) { return 1.0f / sqrtf(var[c] + eps); }
__device__ __forceinline__ void channel_consts(const BnAffine& f, int c, float& mean, float& a, float& b,
                                               float* invstd = nullptr) {
    const float is = bn_invstd(f.var, f.eps, c);
    mean = f.mean[c];
    a = f.weight[c] * is;
    b = f.bias[c];
    if (invstd) *invstd = is;
}

// ---- channels-last lane ------------------------------------------------------------------------------------------
// Memory order [N, H*W, C].  A thread owns FOUR consecutive channels c0 .. c0 + 3 (one 4-element access) and walks
// items (pixels, pooled pixels, quads) with a grid stride; the C / 4 threads of an item read one contiguous segment.
// CONTRACT: C % 4 == 0 and 1024 % C == 0 (nhwc_channels_ok), workgroups of 256 threads: then a thread's channel group
// never changes, its constants live in registers, a workgroup covers rows = 256 / (C / 4) items per trip, and thread
// `prow * groups + cg` takes item  blockIdx.x * rows + prow + trip * gridDim.x * rows.  That walk is the first stage of
// the summation order of the channel sums.
struct NhwcLane {
    int groups, rows, prow, c0;
    float mean[4], a[4], b[4];
    __device__ __forceinline__ int64_t first() const { return (int64_t)blockIdx.x * rows + prow; }
    __device__ __forceinline__ int64_t stride() const { return (int64_t)gridDim.x * rows; }
};
__device__ __forceinline__ NhwcLane nhwc_lane(const BnAffine& f, int C) {
    NhwcLane l;
    l.groups = C >> 2;
    l.rows = 256 / l.groups;
    l.prow = threadIdx.x / l.groups;
    l.c0 = 4 * (threadIdx.x % l.groups);
#pragma unroll
    for (int i = 0; i < 4; i++) channel_consts(f, l.c0 + i, l.mean[i], l.a[i], l.b[i]);
    return l;
}

// ---- block sums ---------------------------------------------------------------------------------------------------
// The backward kernels reduce K per-channel sums (sum g, sum g * d [, sum g * dd]) without atomics: each thread sums its
// elements in walk order, the workgroup combines them in a fixed order into one slot, and bn_finish_kernel sums the
// slots.  Partial layout: partial[k][C][slots].  All threads of the workgroup must call these (they synchronise).

// Channels-last.  CONTRACT: LDS row stride 4 K + 1 floats (9 / 13: conflict-free column reads); the first `groups`
// threads add the rows of their channel group in ASCENDING row order starting from 0; slot = blockIdx.x of gridDim.x.
template <int K>
__device__ __forceinline__ void nhwc_block_sums(const NhwcLane& l, const float (&s)[K][4], float* partial, int C) {
    __shared__ float red[256][4 * K + 1];
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int i = 0; i < 4; i++) red[threadIdx.x][4 * k + i] = s[k][i];
    __syncthreads();
    if (threadIdx.x < l.groups) {
        float t[4 * K];
#pragma unroll
        for (int i = 0; i < 4 * K; i++) t[i] = 0.0f;
        for (int r = 0; r < l.rows; r++)
#pragma unroll
            for (int i = 0; i < 4 * K; i++) t[i] += red[r * l.groups + threadIdx.x][i];
#pragma unroll
        for (int k = 0; k < K; k++)
#pragma unroll
            for (int i = 0; i < 4; i++) partial[(int64_t)(k * C + l.c0 + i) * gridDim.x + blockIdx.x] = t[4 * k + i];
    }
}

// One channel per workgroup (NCHW kernels, finish kernel).  CONTRACT: within a wave __shfl_down by 32, 16, .. 1, then
// the four waves as (w0 + w1) + (w2 + w3).  The totals are valid on thread 0 only.
template <int K>
__device__ __forceinline__ void wave_block_sums(const float (&s)[K], float (&total)[K]) {
    __shared__ float red[K][4];
#pragma unroll
    for (int k = 0; k < K; k++) {
        float v = s[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) total[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}

// ---- finish kernel ------------------------------------------------------------------------------------------------
// One workgroup per channel sums partial[k][c][0 .. slots) for K = 2 (bn_act, stem_pool) or 3 (bn_add_bn_act):
//   grad_bias = sum 0 (K = 3: also grad_bias_d),  grad_weight = invstd * sum 1,  K = 3: grad_weight_d = invstd_d * sum 2.
// CONTRACT: thread t adds slots t, t + 256, .. in that order, then wave_block_sums, and the multiplication by invstd
// comes LAST.  NULL outputs are skipped.  (A template: the header is included by two translation units.)
struct BnFinishOut {
    const float* var;   float eps;   float* grad_weight;   float* grad_bias;
    const float* var_d; float eps_d; float* grad_weight_d; float* grad_bias_d;   // K = 3 only
};
// (value-initialised, then filled, like bn_affine)
static inline BnFinishOut bn_finish_out(const float* var, float eps, float* grad_weight, float* grad_bias, const float* var_d = nullptr,
                                        float eps_d = 0.0f, float* grad_weight_d = nullptr, float* grad_bias_d = nullptr) {
    BnFinishOut o{};
    o.var = var; o.eps = eps; o.grad_weight = grad_weight; o.grad_bias = grad_bias;
    o.var_d = var_d; o.eps_d = eps_d; o.grad_weight_d = grad_weight_d; o.grad_bias_d = grad_bias_d;
    return o;
}
template <int K>
__global__ __launch_bounds__(256) void bn_finish_kernel(const float* __restrict__ partial, int64_t slots, int C, BnFinishOut o) {
    static_assert(K == 2 || K == 3, "two or three sums per channel");
    const int c = blockIdx.x;
    float s[K], t[K];
#pragma unroll
    for (int k = 0; k < K; k++) s[k] = 0.0f;
    for (int64_t j = threadIdx.x; j < slots; j += 256)
#pragma unroll
        for (int k = 0; k < K; k++) s[k] += partial[((int64_t)k * C + c) * slots + j];
    wave_block_sums<K>(s, t);
    if (threadIdx.x == 0) {
        if (o.grad_bias) o.grad_bias[c] = t[0];
        if (K == 3 && o.grad_bias_d) o.grad_bias_d[c] = t[0];
        if (o.grad_weight) o.grad_weight[c] = t[1] * bn_invstd(o.var, o.eps, c);
        if (K == 3 && o.grad_weight_d) o.grad_weight_d[c] = t[K - 1] * bn_invstd(o.var_d, o.eps_d, c);
    }
}

// ---- host helpers -------------------------------------------------------------------------------------------------
// the channel-count rule of the channels-last kernels (see NhwcLane)
static inline bool nhwc_channels_ok(int C) { return C >= 4 && C <= 1024 && (1024 % C) == 0; }

// Workgroups of a channels-last launch over `items`: one per 256 / (C / 4) items, at least 1, at most `cap` (beyond it
// the kernels take further grid-stride trips).  CONTRACT: the count is the grid AND the number of partial-sum slots, so
// it and the family's cap fix the bits of grad_weight / grad_bias.
static inline int nhwc_blocks(int64_t items, int C, int cap) {
    const int rows = 256 / (C / 4);
    const int64_t need = (items + rows - 1) / rows;
    return (int)(need < cap ? (need < 1 ? 1 : need) : cap);
}

// may `p` be the base of 4-element accesses of this activation type (16 bytes fp32, 8 bytes bf16)?  NULL may.
static inline bool aligned4(const void* p, int act_dtype) {
    return !misaligned({p}, act_dtype == 0 ? 15 : 7);
}

// bytes of a workspace for K sums per channel in `slots` slots
static inline int64_t partial_bytes(int K, int C, int64_t slots) { return (int64_t)K * C * slots * 4 + 16; }

// an empty batch: the parameter gradients that were asked for are zero
static inline int zero_param_grads(std::initializer_list<float*> grads, int C, hipStream_t s) {
    for (float* g : grads)
        if (g) {
            const hipError_t e = hipMemsetAsync(g, 0, (size_t)C * 4, s);
            if (e != hipSuccess) return (int)e;
        }
    return MR_OK;
}

// act_dtype (0 fp32, 1 bf16; validated by the caller) -> f(ActType<float>{}) or f(ActType<bf16_t>{}); in the lambda:
// `using T = typename decltype(tag)::type;`
template <typename T> struct ActType { typedef T type; };
template <typename F>
static inline void dispatch_act(int act_dtype, F&& f) {
    if (act_dtype == 0) f(ActType<float>{});
    else f(ActType<bf16_t>{});
}

template <int K>
static inline int launch_bn_finish(const float* partial, int64_t slots, int C, const BnFinishOut& o, hipStream_t s) {
    hipLaunchKernelGGL(bn_finish_kernel<K>, dim3((unsigned)C), dim3(256), 0, s, partial, slots, C, o);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

}  // namespace mr
