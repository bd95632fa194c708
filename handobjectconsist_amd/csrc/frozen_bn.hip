// frozen_bn.hip -- BatchNorm with frozen statistics fused with the residual add and the ReLU that follow it,
// forward and backward, for gfx950 (the trainer side of SURVEY 8f "f2").
//
// The reference trains with --freeze_batchnorm (trainmeshwarp.py:205-206, 237-240: BatchNorm layers in eval mode,
// affine parameters trainable), so every BN of the ResNet-18 trunk (resnet.py:31-60, 140-175) is the per-channel
// affine map  z = (x - mean) * (weight / sqrt(var + eps)) + bias,  followed by  out = relu(z)  or
// out = relu(z + identity)  (resnet.py:46-58) or nothing (the down-sampling branch).  Stock PyTorch runs that as
// 2 - 3 element-wise kernels forward and a generic batch_norm_backward_kernel + threshold_backward in the backward:
// 10.7 ms of a 42 ms step, streaming 2.5 GB of activations several times at ~2 TB/s.  Here: ONE pass forward
// (read x [, identity], write out) and ONE pass backward (read grad_out, x [, identity]; write grad_x [, grad of the
// identity]; reduce grad_weight / grad_bias), 16-byte accesses.
//
// Work split: a workgroup owns ONE channel and a range of samples, so the channel constants are wave-uniform
// scalars and the two reductions of the backward finish inside the workgroup; per-(channel, range) partial sums
// are combined by a second tiny kernel in a fixed order (deterministic, no float atomics).
// The ReLU mask is recomputed in the backward from x (and the identity) with the forward's exact expression.
//
// Activation I/O, channel constants, the channels-last lane, the block sums, the finish kernel and the host helpers
// are bn_device.hpp's, shared with stem_pool.hip; the contracts that keep results bit-stable are stated there.
#include "bn_device.hpp"

namespace mr {

struct BnParams {
    const void* x;          // [N,C,HW]  fp32 or bf16 (the activation type T of the kernel)
    const void* residual;   // [N,C,HW] or NULL
    BnAffine bn;
    int relu;
    int N, C, HW, split;    // split = sample ranges per channel
    // forward
    void* y;
    // backward
    const void* grad_y;
    const void* grad_y2;    // optional second gradient of y (y feeds two consumers): summed on load
    void* grad_x;
    void* grad_residual;    // NULL or [N,C,HW]
    float* partial;         // [2][C][slots]: sum g, sum g * (x - mean)
};

// One element, either direction.  CONTRACT (expression shapes): d = x - mean;  z = d * a + b;  z = z + residual;
// forward out = relu ? relu_nan(z) : z;  backward g = (relu && !(z > 0)) ? 0 : grad, grad_residual = g, out = g * a,
// sum_g += g, sum_gd += g * d.
template <bool BACKWARD>
__device__ __forceinline__ void bn_act_element(float x, bool has_res, float res, float grad, bool relu, float mean, float a,
                                               float b, float& out, float& gres, float& sum_g, float& sum_gd) {
    const float d = x - mean;
    float z = d * a + b;
    if (has_res) z = z + res;
    if (!BACKWARD) {
        out = relu ? relu_nan(z) : z;
    } else {
        const float g = (relu && !(z > 0.0f)) ? 0.0f : grad;
        gres = g;
        out = g * a;
        sum_g += g;
        sum_gd += g * d;
    }
}

// grid = C * split workgroups of 256 threads; workgroup (c, k) covers samples [k * N / split, (k + 1) * N / split)
template <typename T, bool VEC, bool BACKWARD>
__global__ __launch_bounds__(256) void bn_act_kernel(BnParams p) {
    const int c = blockIdx.x / p.split, k = blockIdx.x % p.split;
    const int n0 = (int)((int64_t)k * p.N / p.split), n1 = (int)((int64_t)(k + 1) * p.N / p.split);
    float mean, a, b;
    channel_consts(p.bn, c, mean, a, b);
    constexpr int W = VEC ? 4 : 1;
    const int per_plane = p.HW / W;                 // VEC: HW % 4 == 0
    const unsigned total = (unsigned)(n1 - n0) * (unsigned)per_plane;  // < 2^31, checked by the host
    const bool relu = p.relu != 0, has_res = p.residual != nullptr;
    float s[2] = {0.0f, 0.0f};
    for (unsigned e = threadIdx.x; e < total; e += 256) {
        const unsigned q = e / (unsigned)per_plane;
        const int n = n0 + (int)q, j = (int)(e - q * (unsigned)per_plane);
        const int64_t o = ((int64_t)n * p.C + c) * p.HW + (int64_t)j * W;
        float xv[W], rv[W] = {}, gv[W] = {}, out[W], gres[W];
        if (VEC) {
            load4<T>(p.x, o, xv);
            if (has_res) load4<T>(p.residual, o, rv);
            if (BACKWARD) load4_grad<T>(p.grad_y, p.grad_y2, o, gv);
        } else {
            xv[0] = load1<T>(p.x, o);
            if (has_res) rv[0] = load1<T>(p.residual, o);
            if (BACKWARD) gv[0] = load1_grad<T>(p.grad_y, p.grad_y2, o);
        }
#pragma unroll
        for (int i = 0; i < W; i++) bn_act_element<BACKWARD>(xv[i], has_res, rv[i], gv[i], relu, mean, a, b, out[i], gres[i], s[0], s[1]);
        void* dst = BACKWARD ? p.grad_x : p.y;
        if (VEC) {
            store4<T>(dst, o, out);
            if (BACKWARD && p.grad_residual) store4<T>(p.grad_residual, o, gres);
        } else {
            store1<T>(dst, o, out[0]);
            if (BACKWARD && p.grad_residual) store1<T>(p.grad_residual, o, gres[0]);
        }
    }
    if (BACKWARD && p.partial) {
        float t[2];
        wave_block_sums<2>(s, t);
        if (threadIdx.x == 0) {
            p.partial[(int64_t)c * p.split + k] = t[0];
            p.partial[(int64_t)(p.C + c) * p.split + k] = t[1];
        }
    }
}

// ---- channels-last (NHWC) activations: memory order [N, H*W, C] --------------------------------------------
// MIOpen's convolutions are faster on channels-last tensors (no NCHW<->NHWC transposes around its implicit-GEMM
// kernels: 23.5 instead of 26.9 ms per step for the trunk's convolutions, scripts/conv_layout.py), so the glue
// kernels come in that layout too: one NhwcLane per thread, per-thread partial sums combined once per workgroup
// (nhwc_block_sums), workgroup partials [C][blocks] summed by bn_finish_kernel.
constexpr int BN_NHWC_BLOCKS = 2048;

template <typename T, bool BACKWARD>
__global__ __launch_bounds__(256) void bn_act_nhwc_kernel(BnParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C);
    const int64_t pixels = (int64_t)p.N * p.HW;
    const bool relu = p.relu != 0, has_res = p.residual != nullptr;
    float s[2][4] = {};
    for (int64_t px = l.first(); px < pixels; px += l.stride()) {
        const int64_t o = px * p.C + l.c0;
        float xv[4], rv[4] = {}, gv[4] = {}, out[4], gres[4];
        load4<T>(p.x, o, xv);
        if (has_res) load4<T>(p.residual, o, rv);
        if (BACKWARD) load4_grad<T>(p.grad_y, p.grad_y2, o, gv);
#pragma unroll
        for (int i = 0; i < 4; i++)
            bn_act_element<BACKWARD>(xv[i], has_res, rv[i], gv[i], relu, l.mean[i], l.a[i], l.b[i], out[i], gres[i], s[0][i], s[1][i]);
        store4<T>(BACKWARD ? p.grad_x : p.y, o, out);
        if (BACKWARD && p.grad_residual) store4<T>(p.grad_residual, o, gres);
    }
    if (BACKWARD && p.partial) nhwc_block_sums<2>(l, s, p.partial, p.C);
}

// ---- a block's tail with its downsample branch: relu(bn(x) + bn_d(xd)), NHWC ------------------------------------------
// The first block of layers 2 - 4 ends in  r = bn_d(conv_d(..));  y = relu(bn2(conv2(..)) + r).  As two bn_act launches
// r is written, read back, its gradient written and read back again; here both affine maps run in one pass each way
// (5 tensor streams and a launch + a finish launch less per block).  Same expression shape as the two kernels it
// replaces -- r = dd * ad + bd;  z = d * a + b;  z = z + r -- so fp32 results have the same bits; for bf16
// activations r is no longer rounded to bf16 in between.  Backward: g = z > 0 ? grad_y [+ grad_y2] : 0;
// grad_x = g * a, grad_xd = g * ad; sums g (both biases), g * d, g * dd.  Same pixel walk, workgroup count and
// summation order as bn_act_nhwc_kernel, so the parameter gradients keep their bits too.
struct BnAddParams {
    const void* x;          // [N,HW,C] main branch (conv2's output)
    const void* xd;         // [N,HW,C] downsample branch (conv_d's output)
    BnAffine bn, bn_d;
    int N, C, HW;
    void* y;
    const void* grad_y;
    const void* grad_y2;    // optional second gradient of y: summed on load
    void* grad_x;
    void* grad_xd;
    float* partial;         // [3][C][workgroups]: sum g, sum g * (x - mean), sum g * (xd - mean_d)
};

template <typename T, bool BACKWARD>
__global__ __launch_bounds__(256) void bn_add_bn_act_nhwc_kernel(BnAddParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C), ld = nhwc_lane(p.bn_d, p.C);
    const int64_t pixels = (int64_t)p.N * p.HW;
    float s[3][4] = {};
    for (int64_t px = l.first(); px < pixels; px += l.stride()) {
        const int64_t o = px * p.C + l.c0;
        float xv[4], dv[4], gv[4], out[4], outd[4];
        load4<T>(p.x, o, xv);
        load4<T>(p.xd, o, dv);
        if (BACKWARD) load4_grad<T>(p.grad_y, p.grad_y2, o, gv);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float dd = dv[i] - ld.mean[i];
            const float r = dd * ld.a[i] + ld.b[i];
            const float d = xv[i] - l.mean[i];
            float z = d * l.a[i] + l.b[i];
            z = z + r;
            if (!BACKWARD) {
                out[i] = relu_nan(z);
            } else {
                const float g = !(z > 0.0f) ? 0.0f : gv[i];
                out[i] = g * l.a[i];
                outd[i] = g * ld.a[i];
                s[0][i] += g;
                s[1][i] += g * d;
                s[2][i] += g * dd;
            }
        }
        store4<T>(BACKWARD ? p.grad_x : p.y, o, out);
        if (BACKWARD) store4<T>(p.grad_xd, o, outd);
    }
    if (BACKWARD && p.partial) nhwc_block_sums<3>(l, s, p.partial, p.C);
}

// sample ranges per channel: enough workgroups to fill the chip (>= ~4096), never more than N
static inline int bn_split(int N, int C) {
    int s = (4096 + C - 1) / C;
    if (s < 1) s = 1;
    if (s > N) s = N;
    return s;
}

// Partial-sum slots per channel of one bn_act backward call = the workgroups per channel that write them: bn_split for
// NCHW, the capped workgroup count for channels-last.  pixels < 0: the call is not known (workspace sizing, which gets
// neither the plane nor the layout) -> the most that any call with this N and C can need.
static inline int64_t bn_act_slots(int N, int C, int channels_last, int64_t pixels) {
    const int64_t split = bn_split(N > 0 ? N : 1, C > 0 ? C : 1);
    if (pixels < 0) return split > BN_NHWC_BLOCKS ? split : BN_NHWC_BLOCKS;
    return channels_last ? nhwc_blocks(pixels, C, BN_NHWC_BLOCKS) : split;
}
// bn_add_bn_act (channels-last only), same convention
static inline int64_t bn_add_slots(int C, int64_t pixels) {
    return pixels < 0 ? BN_NHWC_BLOCKS : nhwc_blocks(pixels, C, BN_NHWC_BLOCKS);
}

// the NCHW kernel or, channels_last, the NHWC kernel on `blocks` workgroups
template <bool BACKWARD>
static void bn_launch(const BnParams& p, int act_dtype, int channels_last, bool vec, int blocks, hipStream_t s) {
    dispatch_act(act_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const dim3 grid((unsigned)p.C * p.split);
        if (channels_last) hipLaunchKernelGGL((bn_act_nhwc_kernel<T, BACKWARD>), dim3((unsigned)blocks), dim3(256), 0, s, p);
        else if (vec) hipLaunchKernelGGL((bn_act_kernel<T, true, BACKWARD>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((bn_act_kernel<T, false, BACKWARD>), grid, dim3(256), 0, s, p);
    });
}

static BnParams bn_fill(const void* x, const void* residual, const float* weight, const float* bias, const float* mean,
                        const float* var, float eps, int relu, int N, int C, int plane) {
    BnParams p{};
    p.x = x; p.residual = residual; p.bn = bn_affine(weight, bias, mean, var, eps);
    p.relu = relu; p.N = N; p.C = C; p.HW = plane; p.split = bn_split(N, C);
    return p;
}
// the NCHW kernel's 32-bit element counter and grid
static inline bool bn_sizes_ok(const BnParams& p) {
    return (int64_t)p.C * p.split <= 0x7fffffff && ((int64_t)p.N / p.split + 1) * p.HW <= 0x7fffffff;
}

}  // namespace mr

extern "C" int mr_bn_act_forward(const void* x, const void* residual, const float* weight, const float* bias,
                                 const float* running_mean, const float* running_var, float eps, int relu, int act_dtype,
                                 int channels_last, void* y, int batch_size, int channels, int plane,
                                 mr_stream_t stream) {
    using namespace mr;
    if (batch_size < 0 || channels < 0 || plane < 0 || (act_dtype != 0 && act_dtype != 1)) return MR_ERR_BADARG;
    if (channels_last && channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    if (batch_size == 0 || channels == 0 || plane == 0) return MR_OK;
    if (!x || !weight || !bias || !running_mean || !running_var || !y) return MR_ERR_BADARG;
    BnParams p = bn_fill(x, residual, weight, bias, running_mean, running_var, eps, relu, batch_size, channels, plane);
    p.y = y;
    if (!bn_sizes_ok(p)) return MR_ERR_BADARG;
    const bool all_aligned = aligned4(x, act_dtype) && aligned4(y, act_dtype) && aligned4(residual, act_dtype);
    if (channels_last && !all_aligned) return MR_ERR_BADARG;
    const int blocks = channels_last ? nhwc_blocks((int64_t)batch_size * plane, channels, BN_NHWC_BLOCKS) : 0;
    bn_launch<false>(p, act_dtype, channels_last, plane % 4 == 0 && all_aligned, blocks, (hipStream_t)stream);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int64_t mr_bn_act_backward_workspace_bytes(int batch_size, int channels) {
    if (batch_size < 0 || channels < 0) return -1;
    return mr::partial_bytes(2, channels, mr::bn_act_slots(batch_size, channels, 0, -1));
}

extern "C" int mr_bn_act_backward(const void* grad_y, const void* grad_y2, const void* x, const void* residual,
                                  const float* weight,
                                  const float* bias, const float* running_mean, const float* running_var, float eps,
                                  int relu, int act_dtype, int channels_last, void* grad_x, void* grad_residual,
                                  float* grad_weight, float* grad_bias, void* workspace, int64_t workspace_bytes,
                                  int batch_size, int channels, int plane, mr_stream_t stream) {
    using namespace mr;
    if (batch_size < 0 || channels < 0 || plane < 0 || (act_dtype != 0 && act_dtype != 1)) return MR_ERR_BADARG;
    if (channels_last && channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    if (channels == 0) return MR_OK;
    if (!weight || !bias || !running_mean || !running_var) return MR_ERR_BADARG;
    const bool want_params = grad_weight || grad_bias;
    if (batch_size == 0 || plane == 0) return zero_param_grads({grad_weight, grad_bias}, channels, (hipStream_t)stream);
    if (!grad_y || !x || !grad_x) return MR_ERR_BADARG;
    if (grad_residual && !residual) return MR_ERR_BADARG;
    if (want_params && (!workspace || workspace_bytes < mr_bn_act_backward_workspace_bytes(batch_size, channels)))
        return MR_ERR_BADARG;
    BnParams p = bn_fill(x, residual, weight, bias, running_mean, running_var, eps, relu, batch_size, channels, plane);
    p.grad_y = grad_y; p.grad_y2 = grad_y2; p.grad_x = grad_x; p.grad_residual = grad_residual;
    p.partial = want_params ? static_cast<float*>(workspace) : nullptr;
    if (!bn_sizes_ok(p)) return MR_ERR_BADARG;
    const bool all_aligned = aligned4(x, act_dtype) && aligned4(grad_y, act_dtype) && aligned4(grad_y2, act_dtype) &&
                             aligned4(grad_x, act_dtype) && aligned4(residual, act_dtype) && aligned4(grad_residual, act_dtype);
    if (channels_last && !all_aligned) return MR_ERR_BADARG;
    const int64_t slots = bn_act_slots(batch_size, channels, channels_last, (int64_t)batch_size * plane);
    bn_launch<true>(p, act_dtype, channels_last, plane % 4 == 0 && all_aligned, (int)slots, (hipStream_t)stream);
    MR_CHECK_LAUNCH();
    if (!want_params) return MR_OK;
    return launch_bn_finish<2>(p.partial, slots, channels, bn_finish_out(running_var, eps, grad_weight, grad_bias), (hipStream_t)stream);
}

namespace mr {
static BnAddParams bn_add_fill(const void* x, const void* xd, const BnAffine& bn, const BnAffine& bn_d, int N, int C, int plane) {
    BnAddParams p{};
    p.x = x; p.xd = xd; p.bn = bn; p.bn_d = bn_d; p.N = N; p.C = C; p.HW = plane;
    return p;
}
template <bool BACKWARD>
static void bn_add_launch(const BnAddParams& p, int act_dtype, int blocks, hipStream_t s) {
    dispatch_act(act_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((bn_add_bn_act_nhwc_kernel<T, BACKWARD>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    });
}
}  // namespace mr

extern "C" int mr_bn_add_bn_act_forward(const void* x, const void* xd, const float* weight, const float* bias,
                                        const float* running_mean, const float* running_var, float eps,
                                        const float* weight_d, const float* bias_d, const float* running_mean_d,
                                        const float* running_var_d, float eps_d, int act_dtype, void* y, int batch_size,
                                        int channels, int plane, mr_stream_t stream) {
    using namespace mr;
    if (batch_size < 0 || channels < 0 || plane < 0 || (act_dtype != 0 && act_dtype != 1)) return MR_ERR_BADARG;
    if (channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    if (batch_size == 0 || channels == 0 || plane == 0) return MR_OK;
    if (!x || !xd || !weight || !bias || !running_mean || !running_var || !weight_d || !bias_d || !running_mean_d ||
        !running_var_d || !y)
        return MR_ERR_BADARG;
    if (!aligned4(x, act_dtype) || !aligned4(xd, act_dtype) || !aligned4(y, act_dtype)) return MR_ERR_BADARG;
    BnAddParams p = bn_add_fill(x, xd, bn_affine(weight, bias, running_mean, running_var, eps),
                                bn_affine(weight_d, bias_d, running_mean_d, running_var_d, eps_d), batch_size, channels, plane);
    p.y = y;
    bn_add_launch<false>(p, act_dtype, nhwc_blocks((int64_t)batch_size * plane, channels, BN_NHWC_BLOCKS), (hipStream_t)stream);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int64_t mr_bn_add_bn_act_backward_workspace_bytes(int batch_size, int channels) {
    if (batch_size < 0 || channels < 0) return -1;
    return mr::partial_bytes(3, channels, mr::bn_add_slots(channels, -1));
}

extern "C" int mr_bn_add_bn_act_backward(const void* grad_y, const void* grad_y2, const void* x, const void* xd,
                                         const float* weight, const float* bias, const float* running_mean,
                                         const float* running_var, float eps, const float* weight_d, const float* bias_d,
                                         const float* running_mean_d, const float* running_var_d, float eps_d,
                                         int act_dtype, void* grad_x, void* grad_xd, float* grad_weight, float* grad_bias,
                                         float* grad_weight_d, float* grad_bias_d, void* workspace,
                                         int64_t workspace_bytes, int batch_size, int channels, int plane,
                                         mr_stream_t stream) {
    using namespace mr;
    if (batch_size < 0 || channels < 0 || plane < 0 || (act_dtype != 0 && act_dtype != 1)) return MR_ERR_BADARG;
    if (channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    if (channels == 0) return MR_OK;
    if (!weight || !bias || !running_mean || !running_var || !weight_d || !bias_d || !running_mean_d || !running_var_d)
        return MR_ERR_BADARG;
    const bool want_params = grad_weight || grad_bias || grad_weight_d || grad_bias_d;
    if (batch_size == 0 || plane == 0)
        return zero_param_grads({grad_weight, grad_bias, grad_weight_d, grad_bias_d}, channels, (hipStream_t)stream);
    if (!grad_y || !x || !xd || !grad_x || !grad_xd) return MR_ERR_BADARG;
    if (want_params && (!workspace || workspace_bytes < mr_bn_add_bn_act_backward_workspace_bytes(batch_size, channels)))
        return MR_ERR_BADARG;
    if (!aligned4(x, act_dtype) || !aligned4(xd, act_dtype) || !aligned4(grad_y, act_dtype) || !aligned4(grad_y2, act_dtype) ||
        !aligned4(grad_x, act_dtype) || !aligned4(grad_xd, act_dtype))
        return MR_ERR_BADARG;
    BnAddParams p = bn_add_fill(x, xd, bn_affine(weight, bias, running_mean, running_var, eps),
                                bn_affine(weight_d, bias_d, running_mean_d, running_var_d, eps_d), batch_size, channels, plane);
    p.grad_y = grad_y; p.grad_y2 = grad_y2; p.grad_x = grad_x; p.grad_xd = grad_xd;
    p.partial = want_params ? static_cast<float*>(workspace) : nullptr;
    const int64_t slots = bn_add_slots(channels, (int64_t)batch_size * plane);
    bn_add_launch<true>(p, act_dtype, (int)slots, (hipStream_t)stream);
    MR_CHECK_LAUNCH();
    if (!want_params) return MR_OK;
    return launch_bn_finish<3>(p.partial, slots, channels,
                               bn_finish_out(running_var, eps, grad_weight, grad_bias, running_var_d, eps_d, grad_weight_d, grad_bias_d),
                               (hipStream_t)stream);
}
