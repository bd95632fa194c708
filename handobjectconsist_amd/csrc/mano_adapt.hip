// mano_adapt.hip -- MeshRegNet's ManoAdaptor (meshregnet.py:23-51, used at :192-198) for gfx950 (MI355X): a dense
// [J, V] regressor applied to the POSED hand vertices, then joints and vertices re-centred on one adapted joint.
//
//   j[b,k,:] = sum_i weight[k,i] * verts[b,i,:]        c[b] = j[b,center]  (0 for center == -1)
//   joints_out = j - c                                   verts_out = verts - c
//
// Replaces transpose + Linear + index + two broadcast subtractions and their autograd (about ten launches) by one launch
// each way, plus one for the weight's gradient where it is asked for.  One workgroup of four waves per sample: the sample's
// vertices (12 V bytes) sit in LDS, waves take joints round-robin, the lanes of a wave stride over the vertices with three
// accumulators and are summed by a butterfly, whose order is fixed.  No atomics anywhere; a sample's results depend on
// nothing but that sample.  The whole batch is 3 B J V = 9.4 M multiply-adds at B = 192: fp32 FMA on the vector units.
// Every loop bound is a kernel argument.
#include "mr_common.hpp"

namespace mr {

constexpr int AD_THREADS = 256, AD_WAVES = AD_THREADS / MR_WAVE;
constexpr int AD_MAX_J = 32, AD_MAX_V = 4096;  // the LDS budget: (3 V + 3 J + 15) floats = 49 596 bytes of a workgroup's 64 KB

struct AdaptParams {
    const float* verts;   // [B,V,3]
    const float* weight;  // [J,V]
    int center, V, J;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// grid B, dynamic LDS: sv[3 V] | sj[3 J]
__global__ void __launch_bounds__(AD_THREADS) adapt_forward_kernel(AdaptParams p, float* __restrict__ verts_out,
                                                                   float* __restrict__ joints_out) {
    extern __shared__ float smem[];
    float* sv = smem;
    float* sj = smem + 3 * p.V;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n3 = 3 * p.V;
    const float* v = p.verts + (int64_t)b * n3;
    for (int t = tid; t < n3; t += AD_THREADS) sv[t] = v[t];
    __syncthreads();
    // (lane stride of 3 dwords in LDS: coprime with the 32 banks, no conflict)
    for (int k = wave; k < p.J; k += AD_WAVES) {
        const float* w = p.weight + (int64_t)k * p.V;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 4
        for (int i = lane; i < p.V; i += MR_WAVE) {
            const float wi = w[i];
            a0 = fmaf(wi, sv[3 * i], a0);
            a1 = fmaf(wi, sv[3 * i + 1], a1);
            a2 = fmaf(wi, sv[3 * i + 2], a2);
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
        if (lane == 0) { sj[3 * k] = a0; sj[3 * k + 1] = a1; sj[3 * k + 2] = a2; }
    }
    __syncthreads();
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (p.center >= 0) {
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] = sj[3 * p.center + r];
    }
    // t and t + 256 k differ by k modulo 3 (256 = 3 * 85 + 1): the component walks with the loop
    float* jo = joints_out + (int64_t)b * 3 * p.J;
    for (int t = tid; t < 3 * p.J; t += AD_THREADS) { const int r = t % 3; jo[t] = sj[t] - (r == 0 ? c[0] : r == 1 ? c[1] : c[2]); }
    float* vo = verts_out + (int64_t)b * n3;
    for (int t = tid; t < n3; t += AD_THREADS) { const int r = t % 3; vo[t] = sv[t] - (r == 0 ? c[0] : r == 1 ? c[1] : c[2]); }
}

// Adjoint w.r.t. the vertices.  S[b] = sum_k g_joints[b,k] + sum_i g_verts[b,i] is what flows into c (center >= 0 only):
// gt = g_joints with row `center` reduced by S, grad_verts[b,i] = g_verts[b,i] + sum_k weight[k,i] gt[b,k] (k order).
// grid B, dynamic LDS: sg[3 V] (g_verts, then the result) | sgt[3 J] | red[AD_WAVES][3] | sS[3]
__global__ void __launch_bounds__(AD_THREADS) adapt_backward_kernel(AdaptParams p, const float* __restrict__ g_verts,
                                                                    const float* __restrict__ g_joints,
                                                                    float* __restrict__ gt_out,
                                                                    float* __restrict__ grad_verts) {
    extern __shared__ float smem[];
    float* sg = smem;
    float* sgt = smem + 3 * p.V;
    float* red = sgt + 3 * p.J;
    float* sS = red + 3 * AD_WAVES;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n3 = 3 * p.V, j3 = 3 * p.J;
    for (int t = tid; t < n3; t += AD_THREADS) sg[t] = g_verts ? g_verts[(int64_t)b * n3 + t] : 0.0f;
    for (int t = tid; t < j3; t += AD_THREADS) sgt[t] = g_joints ? g_joints[(int64_t)b * j3 + t] : 0.0f;
    __syncthreads();
    if (p.center >= 0) {
        // vertices: each thread its stride, lanes by the butterfly, waves 0..3 in order; then the joints in k order
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int i = tid; i < p.V; i += AD_THREADS) { a0 += sg[3 * i]; a1 += sg[3 * i + 1]; a2 += sg[3 * i + 2]; }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
        if (lane == 0) { red[3 * wave] = a0; red[3 * wave + 1] = a1; red[3 * wave + 2] = a2; }
        __syncthreads();
        if (tid < 3) {
            float s = red[tid];
            for (int w = 1; w < AD_WAVES; w++) s += red[3 * w + tid];
            for (int k = 0; k < p.J; k++) s += sgt[3 * k + tid];
            sS[tid] = s;
        }
        __syncthreads();
        if (tid < 3) sgt[3 * p.center + tid] -= sS[tid];
        __syncthreads();
    }
    for (int t = tid; t < j3; t += AD_THREADS) gt_out[(int64_t)b * j3 + t] = sgt[t];
    for (int i = tid; i < p.V; i += AD_THREADS) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 4
        for (int k = 0; k < p.J; k++) {
            const float wi = p.weight[(int64_t)k * p.V + i];
            a0 = fmaf(wi, sgt[3 * k], a0);
            a1 = fmaf(wi, sgt[3 * k + 1], a1);
            a2 = fmaf(wi, sgt[3 * k + 2], a2);
        }
        sg[3 * i] += a0; sg[3 * i + 1] += a1; sg[3 * i + 2] += a2;  // (thread i alone touches vertex i)
    }
    __syncthreads();
    for (int t = tid; t < n3; t += AD_THREADS) grad_verts[(int64_t)b * n3 + t] = sg[t];
}

// grad_weight[k,i] = sum_b sum_r gt[b,k,r] verts[b,i,r], b in order: every element is written once, by one thread.
// grid (ceil(V / 256), J)
__global__ void __launch_bounds__(AD_THREADS) adapt_weight_grad_kernel(AdaptParams p, const float* __restrict__ gt, int B,
                                                                       float* __restrict__ grad_weight) {
    const int i = blockIdx.x * AD_THREADS + threadIdx.x, k = blockIdx.y;
    if (i >= p.V) return;
    float acc = 0.0f;
    // (unrolled: eight samples' loads in flight; the chain itself stays in b order)
#pragma unroll 8
    for (int b = 0; b < B; b++) {
        const float* g = gt + ((int64_t)b * p.J + k) * 3;
        const float* v = p.verts + ((int64_t)b * p.V + i) * 3;
        acc = fmaf(g[0], v[0], acc);
        acc = fmaf(g[1], v[1], acc);
        acc = fmaf(g[2], v[2], acc);
    }
    grad_weight[(int64_t)k * p.V + i] = acc;
}

// the backward's one workspace region: gt[B,J,3]
struct AdaptWork {
    int64_t gt, bytes;
};
static AdaptWork adapt_work(int64_t B, int64_t J) {
    AdaptWork w;
    Carve c;
    w.gt = c.take(B * J * 3 * 4, 4);
    w.bytes = c.total();
    return w;
}

// what all three entry points check before anything touches HIP; MR_OK with B == 0 means "nothing to do"
static int adapt_check(int center, int B, int V, int J) {
    if (B < 0 || V < 1 || J < 1 || center < -1 || center >= J) return MR_ERR_BADARG;
    return MR_OK;
}

static AdaptParams adapt_params(const float* verts, const float* weight, int center, int V, int J) {
    AdaptParams p{};  // (value-initialised, then filled: padding bytes are kernel-argument bytes like any other)
    p.verts = verts; p.weight = weight; p.center = center; p.V = V; p.J = J;
    return p;
}

}  // namespace mr

using namespace mr;

extern "C" int mr_mano_adapt_workspace_floats(int batch_size, int num_joints) {
    if (batch_size < 0 || num_joints < 1) return MR_ERR_BADARG;
    const int64_t floats = adapt_work(batch_size, num_joints).bytes / 4;
    return floats <= 0x7fffffffLL ? (int)floats : MR_ERR_BADARG;
}

extern "C" int mr_mano_adapt_forward(const float* verts, const float* weight, int center, float* verts_out, float* joints_out,
                                     int batch_size, int num_verts, int num_joints, mr_stream_t stream) {
    const int rc = adapt_check(center, batch_size, num_verts, num_joints);
    if (rc != MR_OK || batch_size == 0) return rc;
    if (!verts || !weight || !verts_out || !joints_out) return MR_ERR_BADARG;
    if (misaligned({verts, weight, verts_out, joints_out}, 3)) return MR_ERR_BADARG;
    if (num_joints > AD_MAX_J || num_verts > AD_MAX_V) return MR_ERR_NOTIMPL;
    const AdaptParams p = adapt_params(verts, weight, center, num_verts, num_joints);
    const size_t lds = (size_t)(3 * num_verts + 3 * num_joints) * sizeof(float);
    hipLaunchKernelGGL(adapt_forward_kernel, dim3((unsigned)batch_size), dim3(AD_THREADS), lds, (hipStream_t)stream, p, verts_out,
                       joints_out);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_mano_adapt_backward(const float* verts, const float* weight, int center, const float* g_verts,
                                      const float* g_joints, float* work, float* grad_verts, float* grad_weight, int batch_size,
                                      int num_verts, int num_joints, mr_stream_t stream) {
    const int rc = adapt_check(center, batch_size, num_verts, num_joints);
    if (rc != MR_OK || batch_size == 0) return rc;
    if (!verts || !weight || !work || !grad_verts) return MR_ERR_BADARG;
    if (misaligned({verts, weight, g_verts, g_joints, work, grad_verts, grad_weight}, 3)) return MR_ERR_BADARG;
    if (num_joints > AD_MAX_J || num_verts > AD_MAX_V) return MR_ERR_NOTIMPL;
    const AdaptParams p = adapt_params(verts, weight, center, num_verts, num_joints);
    float* gt = at_offset<float>(work, adapt_work(batch_size, num_joints).gt);
    const size_t lds = (size_t)(3 * num_verts + 3 * num_joints + 3 * AD_WAVES + 3) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adapt_backward_kernel, dim3((unsigned)batch_size), dim3(AD_THREADS), lds, s, p, g_verts, g_joints, gt,
                       grad_verts);
    MR_CHECK_LAUNCH();
    if (grad_weight) {
        hipLaunchKernelGGL(adapt_weight_grad_kernel, dim3(blocks1d(num_verts), (unsigned)num_joints), dim3(AD_THREADS), 0, s, p,
                           (const float*)gt, batch_size, grad_weight);
        MR_CHECK_LAUNCH();
    }
    return MR_OK;
}
