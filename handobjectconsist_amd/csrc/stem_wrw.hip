// stem_wrw.hip -- the weight gradient of the stem's 7x7 / stride 2 / padding 3 convolution (3 -> 64 channels), formed
// straight from what the stem's backward holds: the pooled gradient and the layout-2 records of stem_pool.hip.
//
// The composed path writes the gradient of the convolution's output (805 MB at B = 3 x 64, 256 x 256 frames, at least
// 75 % zeros: one pixel per 3 x 3 / stride 2 window receives a gradient) only so that the convolution library's
// weight-gradient kernel can read it back and reduce it to 64 x 3 x 7 x 7 numbers.  Here that map exists per tile in LDS:
//   G[pixel][c]  = a_c * sum of the s of the <= 4 windows whose code names the pixel   (stem_pool_rec_backward_kernel's
//                  arithmetic, same (dy, dx) order;  s = (d * a + b > 0) ? grad_y + grad_y2 : 0)
//   gW[c][tap]  += sum over pixels G[pixel][c] * image[2 cy - 3 + kh][2 cx - 3 + kw][ci],   tap = (kh * 7 + kw) * 3 + ci
// as an fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32) with the pixel index as the reduction dimension: M = 64 channels (two
// blocks of 32), N = 147 taps padded to 160 (five blocks; the padding columns are computed and dropped), K = pixels.
//
// CONTRACT (what fixes the bits of the result; none of it depends on how the grid is scheduled, and there are no atomics):
//   - tiles of SW_TY x SW_TX conv-output pixels of one image, numbered image-major, then row-major; workgroup b of
//     SW_BLOCKS takes tiles b, b + SW_BLOCKS, ... in that order;
//   - wave w of a workgroup takes row w of the tile and feeds its pixels in pairs (s, s + 16), s = 0 .. 15; an MFMA is
//     an fmaf chain in k order, so an accumulator element sums its wave's pixels in exactly that order;
//   - after the last tile the four waves are added as ((w0 + w1) + w2) + w3 into one partial gW per workgroup
//     (workgroups without a tile write zeros), and the finish kernel adds the SW_BLOCKS partials in fp64 as eight runs of
//     64 in ascending order, the runs then in ascending order, and rounds to fp32 once.
#include "bn_device.hpp"

namespace mr {

constexpr int SW_TY = 4, SW_TX = 32;        // conv-output pixels per tile: one row of 32 per wave
constexpr int SW_BLOCKS = 512;              // persistent workgroups = partial results (two per CU of an MI355X)
constexpr int SW_C = 64;                    // output channels: two MFMA row blocks
constexpr int SW_TAPS = 7 * 7 * 3;          // 147
constexpr int SW_NB = 5;                    // tap blocks of 32
constexpr int SW_OUT = SW_C * SW_TAPS;      // 9408 numbers per partial
constexpr int SW_PH = 2 * SW_TY + 5;        // image rows under a tile: 2 cy0 - 3 .. 2 (cy0 + TY - 1) + 3
constexpr int SW_PROW = (2 * SW_TX + 5) * 3;  // floats of an image row under a tile (x, channel interleaved): 207
// LDS row stride of the patch.  213 = 3 * 64 + 21: the offset of tap t from its pixel's first float is then congruent
// to t modulo the 64 banks (kh * 213 + kw * 3 + ci = 21 kh + kw * 3 + ci = t mod 64), so 32 consecutive taps read 32 banks.
constexpr int SW_PW = 213;
constexpr int SW_G = SW_TY * SW_TX * SW_C;  // floats of the gradient tile G[pixel][channel]
constexpr int SW_LDS = SW_G + SW_PH * SW_PW;
constexpr int SW_FIN_RUNS = 8, SW_FIN_RUN = SW_BLOCKS / SW_FIN_RUNS;
static_assert(SW_LDS >= SW_C * SW_NB * 32, "the wave reduction reuses the tile's LDS");
static_assert(SW_OUT % 32 == 0, "finish kernel: 32 outputs per workgroup");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WrwParams {
    const float* grad_y;
    const float* grad_y2;          // optional: summed on load (load4_grad)
    const float* rec_d;            // [N,OH,OW,C]
    const unsigned char* rec_code; // [N,OH,OW,C]
    BnAffine bn;
    const float* image;            // [N,Hin,Win,3]
    float* partial;                // [SW_BLOCKS][C * 147], tap-major: c * 147 + (kh * 7 + kw) * 3 + ci
    int N, Hin, Win, H, W, OH, OW; // H x W: the convolution's output; OH x OW: the pooled map
    int tiles_x, tiles_y;
    int64_t tiles;
};

// The compiler turns "load, then select" back into a branch around the load and waits for every load on its own; a value
// that passes through these stays an unconditional load, and a group of loads issued before the first of them is in flight
// together.
__device__ __forceinline__ void wrw_keep(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void wrw_keep(unsigned& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void wrw_keep(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// 256 threads, two workgroups per CU: 160 accumulator registers + at most 96 others per lane
__global__ __launch_bounds__(256, 2) void stem_conv_wrw_kernel(WrwParams p) {
    __shared__ __attribute__((aligned(16))) float lds[SW_LDS];
    float* const G = lds;
    float* const patch = lds + SW_G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;

    // ---- build phase: a thread owns four channels of the 2 x 2 pixels of a quad (two quads per tile) ----
    const int c0 = 4 * (tid & 15), qcol = tid >> 4;
    float a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float mean;
        channel_consts(p.bn, c0 + i, mean, a[i], b[i]);
    }

    // ---- MFMA phase: lane (half, l31) supplies pixel s + 16 half of the wave's row; A = G[pixel][l31 + 32 m],
    // B = patch[pixel][tap l31 + 32 n].  G's channel index is XORed with 32 for the pixels 16 .. 31 of a row, so that the two
    // halves of a wave read different banks.
    const float* aptr[2];
    const float* bptr[SW_NB];
#pragma unroll
    for (int m = 0; m < 2; m++) aptr[m] = G + (wave * SW_TX + 16 * half) * SW_C + ((l31 + 32 * m) ^ (32 * half));
#pragma unroll
    for (int n = 0; n < SW_NB; n++) {
        const int t = l31 + 32 * n;
        const int off = t < SW_TAPS ? (t / 21) * SW_PW + t % 21 : 0;  // padding taps: any address, the column is dropped
        bptr[n] = patch + 2 * wave * SW_PW + 6 * 16 * half + off;
    }

    f32x16 acc[2][SW_NB];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < SW_NB; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.0f;

    const int per_image = p.tiles_x * p.tiles_y;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int n = (int)(tile / per_image), rem = (int)(tile - (int64_t)n * per_image);
        const int cy0 = (rem / p.tiles_x) * SW_TY, cx0 = (rem % p.tiles_x) * SW_TX;

        // image rows 2 cy0 - 3 .. + 12, columns 2 cx0 - 3 .. + 68; zero outside the image (the convolution's padding).
        // Thread c < 207 takes float c of every row; the loads are unconditional (clamped addresses, then a select), so
        // that all of them are in flight together.
        {
            const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;
            const int c = tid < SW_PROW ? tid : SW_PROW - 1, ix = ix0 + c / 3;
            const bool col = ix >= 0 && ix < p.Win;
            const float* src = p.image + (int64_t)n * p.Hin * p.Win * 3 + (col ? ix0 * 3 + c : 0);
            float pv[SW_PH];
#pragma unroll
            for (int r = 0; r < SW_PH; r++) {
                const int iy = iy0 + r, iyc = iy < 0 ? 0 : (iy >= p.Hin ? p.Hin - 1 : iy);
                pv[r] = src[(int64_t)iyc * p.Win * 3];
            }
#pragma unroll
            for (int r = 0; r < SW_PH; r++) wrw_keep(pv[r]);
#pragma unroll
            for (int r = 0; r < SW_PH; r++) {
                const int iy = iy0 + r;
                if (!col || iy < 0 || iy >= p.Hin) pv[r] = 0.0f;
            }
            if (tid < SW_PROW) {
#pragma unroll
                for (int r = 0; r < SW_PH; r++) patch[r * SW_PW + tid] = pv[r];
            }
        }

        // G of the tile.  Quad (qr, qcol): pixels (cy0 + 2 qr + pr, cx0 + 2 qcol + pc); they lie in the windows
        // (cy0 / 2 + qr + j, cx0 / 2 + qcol + k), j, k in {0, 1}: an even row 2 w in window w only (kh = 1), an odd
        // row 2 w + 1 in windows w + 1 (kh = 0) and w (kh = 2), visited in that order like the kernels of stem_pool.hip.
#pragma unroll 1
        for (int qr = 0; qr < SW_TY / 2; qr++) {
            float s[2][2][4];
            unsigned code[2][2][4];
            // (unconditional loads from clamped windows, then selects: the loads of a quad are in flight together)
            unsigned idw[2][2];
            float4 dv[2][2], g1[2][2], g2[2][2];
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int wy = (cy0 >> 1) + qr + j, wx = (cx0 >> 1) + qcol + k;
                    const int64_t o = (((int64_t)n * p.OH + (wy < p.OH ? wy : p.OH - 1)) * p.OW + (wx < p.OW ? wx : p.OW - 1)) * SW_C + c0;
                    idw[j][k] = *reinterpret_cast<const unsigned*>(p.rec_code + o);
                    dv[j][k] = *reinterpret_cast<const float4*>(p.rec_d + o);
                    g1[j][k] = *reinterpret_cast<const float4*>(p.grad_y + o);
                    g2[j][k] = *reinterpret_cast<const float4*>((p.grad_y2 ? p.grad_y2 : p.grad_y) + o);
                }
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int k = 0; k < 2; k++) { wrw_keep(idw[j][k]); wrw_keep(dv[j][k]); wrw_keep(g1[j][k]); wrw_keep(g2[j][k]); }
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int wy = (cy0 >> 1) + qr + j, wx = (cx0 >> 1) + qcol + k;
                    const bool win = wy < p.OH && wx < p.OW;
                    const float d[4] = {dv[j][k].x, dv[j][k].y, dv[j][k].z, dv[j][k].w};
                    // load4_grad: g = grad_y, then g += grad_y2 when it is present
                    const float gv[4] = {p.grad_y2 ? g1[j][k].x + g2[j][k].x : g1[j][k].x, p.grad_y2 ? g1[j][k].y + g2[j][k].y : g1[j][k].y,
                                         p.grad_y2 ? g1[j][k].z + g2[j][k].z : g1[j][k].z, p.grad_y2 ? g1[j][k].w + g2[j][k].w : g1[j][k].w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        code[j][k][i] = win ? (idw[j][k] >> (8 * i)) & 255u : 255u;  // no window: names no pixel
                        s[j][k][i] = (d[i] * a[i] + b[i] > 0.0f) ? gv[i] : 0.0f;     // ReLU
                    }
                }
#pragma unroll
            for (int pr = 0; pr < 2; pr++)
#pragma unroll
                for (int pc = 0; pc < 2; pc++) {
                    const int py = 2 * qr + pr, px = 2 * qcol + pc;
                    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int dy = 0; dy < 2; dy++) {
                        const int j = pr - dy, kh = pr + 1 - 2 * j;
                        if (j < 0) continue;
#pragma unroll
                        for (int dx = 0; dx < 2; dx++) {
                            const int k = pc - dx, kw = pc + 1 - 2 * k;
                            if (k < 0) continue;
                            const unsigned want = (unsigned)(kh * 3 + kw);
#pragma unroll
                            for (int i = 0; i < 4; i++) g[i] += code[j][k][i] == want ? s[j][k][i] : 0.0f;
                        }
                    }
                    const bool in = cy0 + py < p.H && cx0 + px < p.W;
                    float4 out;
                    out.x = in ? g[0] * a[0] : 0.0f; out.y = in ? g[1] * a[1] : 0.0f;
                    out.z = in ? g[2] * a[2] : 0.0f; out.w = in ? g[3] * a[3] : 0.0f;
                    *reinterpret_cast<float4*>(G + (py * SW_TX + px) * SW_C + (c0 ^ (((px >> 4) & 1) << 5))) = out;
                }
        }
        __syncthreads();

#pragma unroll
        for (int s = 0; s < 16; s++) {
            float av[2], bv[SW_NB];
#pragma unroll
            for (int m = 0; m < 2; m++) av[m] = aptr[m][s * SW_C];
#pragma unroll
            for (int nb = 0; nb < SW_NB; nb++) bv[nb] = bptr[nb][6 * s];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int nb = 0; nb < SW_NB; nb++)
                    acc[m][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[nb], acc[m][nb], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- the four waves, ((w0 + w1) + w2) + w3; every lane adds the elements it holds itself ----
    // (the loop above ends with a barrier, or never ran: the LDS is free)
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
        if (wave == w) {
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int nb = 0; nb < SW_NB; nb++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        float* const slot = lds + ((m * SW_NB + nb) * 16 + r) * 64 + lane;
                        *slot = w > 0 ? *slot + acc[m][nb][r] : acc[m][nb][r];
                    }
        }
        __syncthreads();
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* const out = p.partial + (int64_t)blockIdx.x * SW_OUT;
    for (int e = tid; e < 2 * SW_NB * 16 * 64; e += 256) {
        const int ln = e & 63, r = (e >> 6) & 15, blk = e >> 10, m = blk / SW_NB, nb = blk - m * SW_NB;
        const int c = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), t = 32 * nb + (ln & 31);
        if (t < SW_TAPS) out[c * SW_TAPS + t] = lds[e];
    }
}

// SW_OUT / 32 workgroups; thread (run = tid / 32, e = tid % 32) adds the partials run * 64 .. + 63 of its output in
// ascending order, then thread e adds the eight runs in ascending order.  The partials are added in fp64 and the sum is
// rounded to fp32 once: a workgroup's partial is a small share of the result, so what the fp32 accumulation inside the
// workgroups leaves is small against the one rounding here (a chain of SW_BLOCKS fp32 additions at full magnitude was not:
// 2e-7 of max |gW| on a [4,3,64,64] batch where the convolution library's kernel has 5e-8).
__global__ __launch_bounds__(256) void stem_conv_wrw_finish_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                  int channels_last) {
    __shared__ double red[SW_FIN_RUNS][32];
    const int e = blockIdx.x * 32 + (threadIdx.x & 31), run = threadIdx.x >> 5;
    double v = 0.0;
    for (int j = 0; j < SW_FIN_RUN; j++) v += (double)partial[(int64_t)(run * SW_FIN_RUN + j) * SW_OUT + e];
    red[run][threadIdx.x & 31] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int r = 1; r < SW_FIN_RUNS; r++) t += red[r][threadIdx.x];
        const int c = e / SW_TAPS, tap = e - c * SW_TAPS;
        const int ci = tap % 3, k = tap / 3;  // k = kh * 7 + kw
        out[channels_last ? e : c * SW_TAPS + ci * 49 + k] = (float)t;
    }
}

static bool wrw_geometry(WrwParams& p, int N, int C, int Hin, int Win) {
    if (N < 0 || Hin < 0 || Win < 0 || C != SW_C) return false;
    p.N = N; p.Hin = Hin; p.Win = Win;
    p.H = Hin > 0 ? (Hin - 1) / 2 + 1 : 0;  // (Hin + 2 * 3 - 7) / 2 + 1
    p.W = Win > 0 ? (Win - 1) / 2 + 1 : 0;
    p.OH = p.H > 0 ? (p.H - 1) / 2 + 1 : 0;
    p.OW = p.W > 0 ? (p.W - 1) / 2 + 1 : 0;
    p.tiles_x = (p.W + SW_TX - 1) / SW_TX;
    p.tiles_y = (p.H + SW_TY - 1) / SW_TY;
    p.tiles = (int64_t)N * p.tiles_x * p.tiles_y;
    return true;
}

}  // namespace mr

extern "C" int mr_stem_conv_wrw_tiling(int* tile_height, int* tile_width, int* workgroups) {
    if (tile_height) *tile_height = mr::SW_TY;
    if (tile_width) *tile_width = mr::SW_TX;
    if (workgroups) *workgroups = mr::SW_BLOCKS;
    return MR_OK;
}

extern "C" int64_t mr_stem_conv_wrw_workspace_bytes(int batch_size, int channels, int in_height, int in_width) {
    mr::WrwParams p{};
    if (!mr::wrw_geometry(p, batch_size, channels, in_height, in_width)) return -1;
    return (int64_t)mr::SW_BLOCKS * mr::SW_OUT * 4;
}

extern "C" int mr_stem_conv_wrw(const float* grad_y, const float* grad_y2, const unsigned char* records, const float* weight,
                                const float* bias, const float* running_mean, const float* running_var, float eps,
                                const float* image, float* grad_conv_weight, int weight_channels_last, void* workspace,
                                int64_t workspace_bytes, int batch_size, int channels, int in_height, int in_width,
                                int in_channels, int kernel_size, int stride, int padding, mr_stream_t stream) {
    using namespace mr;
    if (kernel_size != 7 || stride != 2 || padding != 3 || in_channels != 3) return MR_ERR_BADARG;
    WrwParams p{};
    if (!wrw_geometry(p, batch_size, channels, in_height, in_width)) return MR_ERR_BADARG;
    if (!grad_conv_weight) return MR_ERR_BADARG;
    const hipStream_t s = (hipStream_t)stream;
    if (p.tiles == 0) return zero_param_grads({grad_conv_weight}, SW_OUT, s);  // an empty batch: the gradient is zero
    if (!grad_y || !records || !weight || !bias || !running_mean || !running_var || !image) return MR_ERR_BADARG;
    if (!workspace || workspace_bytes < mr_stem_conv_wrw_workspace_bytes(batch_size, channels, in_height, in_width)) return MR_ERR_BADARG;
    // float4 / uchar4 accesses: the record buffer and the gradients on 16 bytes (the code plane follows the d plane, whose
    // size is a multiple of 16 bytes), the workspace and the output on 4
    if (misaligned({records, grad_y, grad_y2}, 15) || misaligned({image, workspace, grad_conv_weight}, 3))
        return MR_ERR_BADARG;
    p.grad_y = grad_y; p.grad_y2 = grad_y2;
    p.rec_d = reinterpret_cast<const float*>(records);
    p.rec_code = records + (int64_t)p.N * p.OH * p.OW * SW_C * 4;
    p.bn = bn_affine(weight, bias, running_mean, running_var, eps);
    p.image = image;
    p.partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(stem_conv_wrw_kernel, dim3(SW_BLOCKS), dim3(256), 0, s, p);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(stem_conv_wrw_finish_kernel, dim3(SW_OUT / 32), dim3(256), 0, s, p.partial, grad_conv_weight,
                       weight_channels_last ? 1 : 0);
    MR_CHECK_LAUNCH();
    return MR_OK;
}
