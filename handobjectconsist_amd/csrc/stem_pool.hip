// stem_pool.hip -- the ResNet stem after its 7x7 convolution, fused: BatchNorm with frozen statistics -> ReLU ->
// MaxPool2d(kernel 3, stride 2, padding 1) (resnet.py:140-147 with --freeze_batchnorm), forward and backward.
//
// Stock PyTorch writes relu(bn(x)) (805 MB at B = 3 x 64, 256 x 256 inputs), reads it back to pool it, keeps it and a
// 64-bit index map for the backward, and runs max_pool_backward (1.46 ms) + batch_norm_backward on top: 3.0 ms of a
// 34 ms step.  Here the full-resolution activation after the BN never exists: the forward reads the convolution
// output once and writes the pooled map (1/4 of the pixels); the backward recomputes z = bn(x) per tile in LDS,
// re-derives every window's arg-max (PyTorch's rule: scan kh, kw ascending, strictly-greater wins, padding ignored)
// and GATHERS the pooled gradient per input pixel -- no atomics, no zero-fill of the 805 MB gradient.
//
// Activation I/O, channel constants, the channels-last lane, the two-gradient load, the block sums, the finish kernel
// and the host helpers are bn_device.hpp's, shared with frozen_bn.hip; the contracts that keep results bit-stable are
// stated there.  The stem's own: z = d * a + b with d = x - mean; the ReLU and the max propagate NaN like torch.relu /
// max_pool2d ("val > max || isnan(val)"); the backward's mask is  z > 0 ? g : 0.
#include "bn_device.hpp"

namespace mr {

struct StemParams {
    const void* x;        // [N,C,H,W] convolution output, fp32 or bf16 (the activation type T of the kernels)
    BnAffine bn;
    int N, C, H, W, OH, OW;   // OH = (H - 1) / 2 + 1
    int tiles_x, tiles_y;
    void* y;              // forward: [N,C,OH,OW]
    const void* grad_y;   // backward
    const void* grad_y2;  // optional second gradient of y (y feeds two consumers): summed on load
    void* grad_x;         // [N,C,H,W]
    float* partial;       // [2][C][N * tiles]: sum g, sum g * (x - mean)   (channels-last: [2][C][workgroups])
    unsigned char* argmax;  // channels-last only: [N,OH,OW,C] arg-max position kh * 3 + kw, written by the forward
};

constexpr int SP_TX = 32, SP_TY = 16;  // windows (= pooled pixels) per tile
// Input region of a tile in LDS: rows 2 oy0 - 1 .. 2 (oy0 + TY) + 1, columns 2 ox0 - 4 .. 2 (ox0 + TX) + 3 -- the
// column range starts 3 pixels early so that it begins on a 16-byte boundary (2 ox0 is a multiple of 64) and can be
// fetched with aligned float4 loads.  LDS row = input row - (2 oy0 - 1), LDS column = input column - (2 ox0 - 4).
constexpr int SP_IH = 2 * SP_TY + 3, SP_IW = 2 * SP_TX + 8, SP_C0 = 4;
constexpr int SP_LDW = SP_IW + 1;

// z = bn(x) (and d = x - mean) of the tile's input region into LDS; -inf / 0 outside the image
template <typename T, bool KEEP_D>
__device__ __forceinline__ void load_tile(const StemParams& p, const T* xp, int oy0, int ox0, float mean, float a,
                                          float b, float (*zt)[SP_LDW], float (*dt)[SP_LDW]) {
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - SP_C0;
    const float ninf = -__builtin_inff();
    if ((p.W & 3) == 0 && (reinterpret_cast<uintptr_t>(xp) & (4 * sizeof(T) - 1)) == 0) {
        for (int e = threadIdx.x; e < SP_IH * (SP_IW / 4); e += 256) {
            const int r = e / (SP_IW / 4), q = e - r * (SP_IW / 4);
            const int iy = iy0 + r, ix = ix0 + 4 * q;  // a float4 is entirely inside or entirely outside the row
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const bool in = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            if (in) load4<T>(xp, (int64_t)iy * p.W + ix, v);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float d = v[i] - mean;
                zt[r][4 * q + i] = in ? d * a + b : ninf;
                if (KEEP_D) dt[r][4 * q + i] = in ? d : 0.0f;
            }
        }
        return;
    }
    for (int e = threadIdx.x; e < SP_IH * SP_IW; e += 256) {
        const int r = e / SP_IW, c = e - r * SP_IW;
        const int iy = iy0 + r, ix = ix0 + c;
        float z = ninf, d = 0.0f;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
            d = load1<T>(xp, (int64_t)iy * p.W + ix) - mean;
            z = d * a + b;
        }
        zt[r][c] = z;
        if (KEEP_D) dt[r][c] = d;
    }
}

// grid = N * C * tiles workgroups of 256 threads
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_forward_kernel(StemParams p) {
    __shared__ float zt[SP_IH][SP_LDW];
    const int tiles = p.tiles_x * p.tiles_y;
    const int plane = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int c = plane % p.C;
    const int oy0 = (t / p.tiles_x) * SP_TY, ox0 = (t % p.tiles_x) * SP_TX;
    float mean, a, b;
    channel_consts(p.bn, c, mean, a, b);
    load_tile<T, false>(p, static_cast<const T*>(p.x) + (int64_t)plane * p.H * p.W, oy0, ox0, mean, a, b, zt, nullptr);
    __syncthreads();
    for (int e = threadIdx.x; e < SP_TY * SP_TX; e += 256) {
        const int wy = e / SP_TX, wx = e % SP_TX;
        const int oy = oy0 + wy, ox = ox0 + wx;
        if (oy >= p.OH || ox >= p.OW) continue;
        float m = 0.0f;  // relu: max(0, max z); every window holds at least one pixel of the image
#pragma unroll
        for (int kh = 0; kh < 3; kh++)
#pragma unroll
            for (int kw = 0; kw < 3; kw++) {
                const float z = zt[2 * wy + kh][2 * wx + kw + SP_C0 - 1];
                m = (z > m || z != z) ? z : m;
            }
        store1<T>(p.y, ((int64_t)plane * p.OH + oy) * p.OW + ox, m);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void stem_pool_backward_kernel(StemParams p) {
    __shared__ float zt[SP_IH][SP_LDW];
    __shared__ float dt[SP_IH][SP_LDW];                 // x - mean of the same region (for grad_weight)
    __shared__ float gw[SP_TY + 1][SP_TX + 1];          // pooled gradient of the tile's windows (+1 row / column)
    __shared__ unsigned char am[SP_TY + 1][SP_TX + 1];  // arg-max position kh * 3 + kw of every window
    const int tiles = p.tiles_x * p.tiles_y;
    const int plane = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int c = plane % p.C;
    const int oy0 = (t / p.tiles_x) * SP_TY, ox0 = (t % p.tiles_x) * SP_TX;
    float mean, a, b;
    channel_consts(p.bn, c, mean, a, b);
    const T* xp = static_cast<const T*>(p.x) + (int64_t)plane * p.H * p.W;
    load_tile<T, true>(p, xp, oy0, ox0, mean, a, b, zt, dt);
    __syncthreads();
    // windows oy0 .. oy0 + TY, ox0 .. ox0 + TX: the owned input rows 2 oy0 .. 2 (oy0 + TY) - 1 touch one window more
    for (int e = threadIdx.x; e < (SP_TY + 1) * (SP_TX + 1); e += 256) {
        const int wy = e / (SP_TX + 1), wx = e - wy * (SP_TX + 1);
        const int oy = oy0 + wy, ox = ox0 + wx;
        float g = 0.0f;
        int best = 0;
        if (oy < p.OH && ox < p.OW) {
            g = load1_grad<T>(p.grad_y, p.grad_y2, ((int64_t)plane * p.OH + oy) * p.OW + ox);
            float mv = -__builtin_inff();  // PyTorch: first strictly greater value of relu(z) in (kh, kw) order, padding skipped
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const float z = zt[2 * wy + k / 3][2 * wx + k % 3 + SP_C0 - 1];
                const float v = relu_nan(z);
                if (z != -__builtin_inff() && (v > mv || v != v)) { mv = v; best = k; }
            }
        }
        gw[wy][wx] = g;
        am[wy][wx] = (unsigned char)best;
    }
    __syncthreads();
    // gather: owned input pixels rows 2 oy0 + [0, 2 TY), columns 2 ox0 + [0, 2 TX); LDS row = input row - (2 oy0 - 1)
    float s[2] = {0.0f, 0.0f};  // sum g, sum g * (x - mean)
    T* gx = static_cast<T*>(p.grad_x) + (int64_t)plane * p.H * p.W;
    const bool vec = (p.W & 3) == 0 && (reinterpret_cast<uintptr_t>(gx) & (4 * sizeof(T) - 1)) == 0;
    for (int e = threadIdx.x; e < 2 * SP_TY * (2 * SP_TX / 4); e += 256) {  // four consecutive owned pixels per item
        const int ry = e / (2 * SP_TX / 4), rx0 = 4 * (e - ry * (2 * SP_TX / 4));
        const int iy = 2 * oy0 + ry, ix0 = 2 * ox0 + rx0;
        if (iy >= p.H || ix0 >= p.W) continue;
        const int ly = ry + 1;  // position relative to the first window's first row
        float out[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int lx = rx0 + i + 1;
            // windows containing the pixel: wy with 2 wy <= ly <= 2 wy + 2, likewise wx
            float g = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
                const int wy = (ly >> 1) - dy;
                const int kh = ly - 2 * wy;
                if (wy < 0 || kh > 2) continue;
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int wx = (lx >> 1) - dx;
                    const int kw = lx - 2 * wx;
                    if (wx < 0 || kw > 2) continue;
                    if (am[wy][wx] == kh * 3 + kw) g += gw[wy][wx];
                }
            }
            const float z = zt[ly][lx + SP_C0 - 1];
            const float gm = (z > 0.0f && ix0 + i < p.W) ? g : 0.0f;  // ReLU
            out[i] = gm * a;
            s[0] += gm;
            s[1] += gm * dt[ly][lx + SP_C0 - 1];
        }
        const int64_t o = (int64_t)iy * p.W + ix0;
        if (vec) {
            store4<T>(gx, o, out);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (ix0 + i < p.W) store1<T>(gx, o + i, out[i]);
        }
    }
    if (p.partial) {
        float total[2];
        wave_block_sums<2>(s, total);
        if (threadIdx.x == 0) {
            const int n = plane / p.C;
            const int64_t per_c = (int64_t)p.N * tiles;
            const int64_t slot = (int64_t)n * tiles + t;
            p.partial[(int64_t)c * per_c + slot] = total[0];
            p.partial[((int64_t)p.C + c) * per_c + slot] = total[1];
        }
    }
}

// ---- channels-last (NHWC) activations ---------------------------------------------------------------------
// A thread owns four consecutive channels of one pixel (one 16-byte access; the C / 4 threads of a pixel read a
// contiguous 4 C-byte segment), so no LDS staging is needed: the forward reads the <= 9 pixels of its window directly
// and also writes each channel's arg-max position (1 byte per pooled value); the backward walks INPUT pixels and
// gathers from the <= 4 windows that contain them by comparing the stored positions -- same arithmetic and tie rule
// as the NCHW kernels.
constexpr int SP_NHWC_BLOCKS = 4096;

template <typename T>
__global__ __launch_bounds__(256) void stem_pool_nhwc_forward_kernel(StemParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C);
    const int64_t total = (int64_t)p.N * p.OH * p.OW;
    for (int64_t op = l.first(); op < total; op += l.stride()) {
        const int ox = (int)(op % p.OW), oy = (int)((op / p.OW) % p.OH), n = (int)(op / ((int64_t)p.OW * p.OH));
        float best[4];
        unsigned bi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; i++) best[i] = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int iy = 2 * oy - 1 + k / 3, ix = 2 * ox - 1 + k % 3;
            if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) continue;
            float xv[4];
            load4<T>(p.x, (((int64_t)n * p.H + iy) * p.W + ix) * p.C + l.c0, xv);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float v = relu_nan((xv[i] - l.mean[i]) * l.a[i] + l.b[i]);
                if (v > best[i] || v != v) { best[i] = v; bi[i] = (unsigned)k; }
            }
        }
        const int64_t o = op * p.C + l.c0;
        store4<T>(p.y, o, best);
        *reinterpret_cast<uchar4*>(p.argmax + o) = make_uchar4((unsigned char)bi[0], (unsigned char)bi[1],
                                                               (unsigned char)bi[2], (unsigned char)bi[3]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void stem_pool_nhwc_backward_kernel(StemParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C);
    const int64_t total = (int64_t)p.N * p.H * p.W;
    float s[2][4] = {};  // sum g, sum g * d
    for (int64_t ip = l.first(); ip < total; ip += l.stride()) {
        const int ix = (int)(ip % p.W), iy = (int)((ip / p.W) % p.H), n = (int)(ip / ((int64_t)p.W * p.H));
        float xv[4], g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4];
        load4<T>(p.x, ip * p.C + l.c0, xv);
        const int ly = iy + 1, lx = ix + 1;  // window w covers l = 2 w .. 2 w + 2
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
            const int wy = (ly >> 1) - dy, kh = ly - 2 * wy;
            if (wy < 0 || wy >= p.OH || kh > 2) continue;
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const int wx = (lx >> 1) - dx, kw = lx - 2 * wx;
                if (wx < 0 || wx >= p.OW || kw > 2) continue;
                const int64_t o = (((int64_t)n * p.OH + wy) * p.OW + wx) * p.C + l.c0;
                const uchar4 id = *reinterpret_cast<const uchar4*>(p.argmax + o);
                float gv[4];
                load4_grad<T>(p.grad_y, p.grad_y2, o, gv);
                const unsigned code = (unsigned)(kh * 3 + kw);
                g[0] += id.x == code ? gv[0] : 0.0f;
                g[1] += id.y == code ? gv[1] : 0.0f;
                g[2] += id.z == code ? gv[2] : 0.0f;
                g[3] += id.w == code ? gv[3] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float d = xv[i] - l.mean[i];
            const float gm = (d * l.a[i] + l.b[i] > 0.0f) ? g[i] : 0.0f;  // ReLU
            out[i] = gm * l.a[i];
            s[0][i] += gm;
            s[1][i] += gm * d;
        }
        store4<T>(p.grad_x, ip * p.C + l.c0, out);
    }
    if (p.partial) nhwc_block_sums<2>(l, s, p.partial, p.C);
}

// ---- channels-last with pooled records (layout code 2) ------------------------------------------------------
// A gradient reaches at most one pixel per pooling window, so the ReLU mask and x - mean matter only there.  The
// forward leaves d = x - mean of every window's arg-max pixel (fp32, also for bf16 activations: the channel sums must
// see the same d as the layouts above) next to its arg-max code; the backward then never touches x:
//   per window    g = grad_y + grad_y2,  s = (d * a + b > 0) ? g : 0        (the expression of the kernels above, same d)
//   per pixel     grad_x = a * sum of the s of the <= 4 windows whose code names the pixel, (dy, dx) order as above
//   per channel   sum s and sum s * d, taken once per window by the thread that owns it
// y and grad_x have the same bits as layouts 0 / 1; grad_weight / grad_bias sum the same terms window by window instead
// of pixel by pixel.  One stated difference: a NaN at a pixel that no window selects used to poison grad_weight through
// 0 * NaN.  Max-pooling propagates NaN, so the windows of a NaN pixel do select a NaN pixel, and the record form sees it
// unless the incoming gradient there is exactly zero.
// Record buffer: d[N,OH,OW,C] fp32, then the codes [N,OH,OW,C] u8 (both planes 16-byte aligned; C % 4 == 0).
__device__ __forceinline__ unsigned char* sp_rec_codes(const StemParams& p) {
    return p.argmax + (int64_t)p.N * p.OH * p.OW * p.C * 4;
}

// A thread produces the 2 x 2 pooled values of its four channels from the 5 x 5 input pixels they share: 25 loads of
// 16 bytes instead of 36.  The pixels are visited row by row, so every window still sees its own in (kh, kw) order.
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_rec_forward_kernel(StemParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C);
    float* rec_d = reinterpret_cast<float*>(p.argmax);
    unsigned char* rec_code = sp_rec_codes(p);
    const int QH = (p.OH + 1) >> 1, QW = (p.OW + 1) >> 1;
    const int64_t total = (int64_t)p.N * QH * QW;
    for (int64_t q = l.first(); q < total; q += l.stride()) {
        const int qx = (int)(q % QW), qy = (int)((q / QW) % QH), n = (int)(q / ((int64_t)QW * QH));
        const int oy0 = 2 * qy, ox0 = 2 * qx;
        float best[2][2][4], bd[2][2][4];
        unsigned bi[2][2][4];
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int i = 0; i < 4; i++) { best[w >> 1][w & 1][i] = -__builtin_inff(); bd[w >> 1][w & 1][i] = 0.0f; bi[w >> 1][w & 1][i] = 0; }
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const int iy = 2 * oy0 - 1 + r;
            if (iy < 0 || iy >= p.H) continue;
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const int ix = 2 * ox0 - 1 + c;
                if (ix < 0 || ix >= p.W) continue;
                float xv[4];
                load4<T>(p.x, (((int64_t)n * p.H + iy) * p.W + ix) * p.C + l.c0, xv);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float d = xv[i] - l.mean[i];
                    const float v = relu_nan(d * l.a[i] + l.b[i]);
#pragma unroll
                    for (int wy = 0; wy < 2; wy++) {
                        const int kh = r - 2 * wy;
                        if (kh < 0 || kh > 2) continue;
#pragma unroll
                        for (int wx = 0; wx < 2; wx++) {
                            const int kw = c - 2 * wx;
                            if (kw < 0 || kw > 2) continue;
                            if (v > best[wy][wx][i] || v != v) { best[wy][wx][i] = v; bd[wy][wx][i] = d; bi[wy][wx][i] = (unsigned)(kh * 3 + kw); }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int wy = 0; wy < 2; wy++)
#pragma unroll
            for (int wx = 0; wx < 2; wx++) {
                const int oy = oy0 + wy, ox = ox0 + wx;
                if (oy >= p.OH || ox >= p.OW) continue;
                const int64_t o = (((int64_t)n * p.OH + oy) * p.OW + ox) * p.C + l.c0;
                store4<T>(p.y, o, best[wy][wx]);
                *reinterpret_cast<float4*>(rec_d + o) = make_float4(bd[wy][wx][0], bd[wy][wx][1], bd[wy][wx][2], bd[wy][wx][3]);
                *reinterpret_cast<uchar4*>(rec_code + o) = make_uchar4((unsigned char)bi[wy][wx][0], (unsigned char)bi[wy][wx][1],
                                                                       (unsigned char)bi[wy][wx][2], (unsigned char)bi[wy][wx][3]);
            }
    }
}

// A thread owns the 2 x 2 input pixels (rows 2 qy - 1, 2 qy; columns 2 qx - 1, 2 qx) that lie in the same four windows
// (qy - 1, qy) x (qx - 1, qx): 4 record loads for 4 pixels instead of 9.  Window (qy, qx) is the thread's own and is the
// only one it counts in the channel sums; the other three are halo.  x is not read.
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_rec_backward_kernel(StemParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C);
    const float* rec_d = reinterpret_cast<const float*>(p.argmax);
    const unsigned char* rec_code = sp_rec_codes(p);
    const int QH = (p.H >> 1) + 1, QW = (p.W >> 1) + 1;
    const int64_t total = (int64_t)p.N * QH * QW;
    float sums[2][4] = {};  // sum s, sum s * d
    for (int64_t q = l.first(); q < total; q += l.stride()) {
        const int qx = (int)(q % QW), qy = (int)((q / QW) % QH), n = (int)(q / ((int64_t)QW * QH));
        float s[2][2][4];
        unsigned code[2][2][4];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int wy = qy - 1 + j, wx = qx - 1 + k;
#pragma unroll
                for (int i = 0; i < 4; i++) { s[j][k][i] = 0.0f; code[j][k][i] = 255u; }  // no window: names no pixel
                if (wy < 0 || wy >= p.OH || wx < 0 || wx >= p.OW) continue;
                const int64_t o = (((int64_t)n * p.OH + wy) * p.OW + wx) * p.C + l.c0;
                const uchar4 id = *reinterpret_cast<const uchar4*>(rec_code + o);
                const float4 dv = *reinterpret_cast<const float4*>(rec_d + o);
                const float d[4] = {dv.x, dv.y, dv.z, dv.w};
                float gv[4];
                load4_grad<T>(p.grad_y, p.grad_y2, o, gv);
                code[j][k][0] = id.x; code[j][k][1] = id.y; code[j][k][2] = id.z; code[j][k][3] = id.w;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float sv = (d[i] * l.a[i] + l.b[i] > 0.0f) ? gv[i] : 0.0f;  // ReLU
                    s[j][k][i] = sv;
                    if (j == 1 && k == 1) { sums[0][i] += sv; sums[1][i] += sv * d[i]; }
                }
            }
#pragma unroll
        for (int pr = 0; pr < 2; pr++) {
            const int iy = 2 * qy - 1 + pr;
            if (iy < 0 || iy >= p.H) continue;
#pragma unroll
            for (int pc = 0; pc < 2; pc++) {
                const int ix = 2 * qx - 1 + pc;
                if (ix < 0 || ix >= p.W) continue;
                float g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4];
#pragma unroll
                for (int dy = 0; dy < 2; dy++) {  // window row qy first (dy = 0), then qy - 1: the order of the kernels above
                    const int kh = pr + 2 * dy;
                    if (kh > 2) continue;
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        const int kw = pc + 2 * dx;
                        if (kw > 2) continue;
                        const unsigned want = (unsigned)(kh * 3 + kw);
#pragma unroll
                        for (int i = 0; i < 4; i++) g[i] += code[1 - dy][1 - dx][i] == want ? s[1 - dy][1 - dx][i] : 0.0f;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) out[i] = g[i] * l.a[i];
                store4<T>(p.grad_x, (((int64_t)n * p.H + iy) * p.W + ix) * p.C + l.c0, out);
            }
        }
    }
    if (p.partial) nhwc_block_sums<2>(l, sums, p.partial, p.C);
}

// The channel sums of the kernel above without its grad_x: for a stem whose input gradient nobody wants (the convolution
// in front of it reads an image, and its weight gradient comes from stem_wrw.hip).  Same walk, same grid, and per thread
// the same additions in the same order -- only a quad's own window (qy, qx) enters the sums -- so grad_weight / grad_bias
// have the bits of the full backward.  Reads d and the gradients; the codes are not needed.
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_rec_sums_kernel(StemParams p) {
    const NhwcLane l = nhwc_lane(p.bn, p.C);
    const float* rec_d = reinterpret_cast<const float*>(p.argmax);
    const int QH = (p.H >> 1) + 1, QW = (p.W >> 1) + 1;
    const int64_t total = (int64_t)p.N * QH * QW;
    float sums[2][4] = {};  // sum s, sum s * d
    for (int64_t q = l.first(); q < total; q += l.stride()) {
        const int qx = (int)(q % QW), qy = (int)((q / QW) % QH), n = (int)(q / ((int64_t)QW * QH));
        if (qy >= p.OH || qx >= p.OW) continue;
        const int64_t o = (((int64_t)n * p.OH + qy) * p.OW + qx) * p.C + l.c0;
        const float4 dv = *reinterpret_cast<const float4*>(rec_d + o);
        const float d[4] = {dv.x, dv.y, dv.z, dv.w};
        float gv[4];
        load4_grad<T>(p.grad_y, p.grad_y2, o, gv);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float sv = (d[i] * l.a[i] + l.b[i] > 0.0f) ? gv[i] : 0.0f;  // ReLU
            sums[0][i] += sv;
            sums[1][i] += sv * d[i];
        }
    }
    nhwc_block_sums<2>(l, sums, p.partial, p.C);
}

static int stem_fill(StemParams& p, const void* x, const float* weight, const float* bias, const float* mean,
                     const float* var, float eps, int N, int C, int H, int W) {
    if (N < 0 || C < 0 || H < 0 || W < 0) return MR_ERR_BADARG;
    p.x = x; p.bn = bn_affine(weight, bias, mean, var, eps);
    p.N = N; p.C = C; p.H = H; p.W = W;
    p.OH = H > 0 ? (H - 1) / 2 + 1 : 0;
    p.OW = W > 0 ? (W - 1) / 2 + 1 : 0;
    p.tiles_x = (p.OW + SP_TX - 1) / SP_TX;
    p.tiles_y = (p.OH + SP_TY - 1) / SP_TY;
    if ((int64_t)N * C * p.tiles_x * p.tiles_y > 0x7fffffff) return MR_ERR_BADARG;
    return MR_OK;
}

// Items the channels-last kernels walk: layout 1 pooled pixels (forward) / input pixels (backward), layout 2 quads of
// 2 x 2 pooled pixels (forward) / the (H / 2 + 1) x (W / 2 + 1) quads of input pixels (backward).
static inline int64_t stem_items(const StemParams& p, int layout, bool backward) {
    if (layout == 2) return backward ? (int64_t)p.N * (p.H / 2 + 1) * (p.W / 2 + 1) : (int64_t)p.N * ((p.OH + 1) / 2) * ((p.OW + 1) / 2);
    return backward ? (int64_t)p.N * p.H * p.W : (int64_t)p.N * p.OH * p.OW;
}

// Partial-sum slots per channel of one backward call = the workgroups per channel that write them: one per (sample, tile)
// in layout 0, the capped workgroup count in layouts 1 and 2.  layout < 0: the call is not known (workspace sizing, which
// does not get the layout) -> the most any layout can need.
static inline int64_t stem_slots(const StemParams& p, int layout) {
    const int64_t nchw = (int64_t)p.N * p.tiles_x * p.tiles_y;
    if (layout < 0) return nchw > SP_NHWC_BLOCKS ? nchw : SP_NHWC_BLOCKS;
    return layout ? nhwc_blocks(stem_items(p, layout, true), p.C, SP_NHWC_BLOCKS) : nchw;
}

// layout code of the entry points' channels_last argument: 0 NCHW, 2 pooled records, anything else layout 1
static inline int stem_layout(int channels_last) { return channels_last == 2 ? 2 : (channels_last ? 1 : 0); }

// the arg-max codes (layout 1: uchar4 accesses) or the record buffer (layout 2: float4 accesses) must be there and aligned
static inline bool stem_records_ok(const unsigned char* argmax, int layout) {
    return argmax && !misaligned({argmax}, layout == 2 ? 15 : 3);
}

template <bool BACKWARD>
static void stem_launch(const StemParams& p, int act_dtype, int layout, int64_t blocks, hipStream_t s) {
    const dim3 grid((unsigned)blocks), block(256);
    dispatch_act(act_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (layout == 2) {
            if (BACKWARD) hipLaunchKernelGGL(stem_pool_rec_backward_kernel<T>, grid, block, 0, s, p);
            else hipLaunchKernelGGL(stem_pool_rec_forward_kernel<T>, grid, block, 0, s, p);
        } else if (layout == 1) {
            if (BACKWARD) hipLaunchKernelGGL(stem_pool_nhwc_backward_kernel<T>, grid, block, 0, s, p);
            else hipLaunchKernelGGL(stem_pool_nhwc_forward_kernel<T>, grid, block, 0, s, p);
        } else {
            if (BACKWARD) hipLaunchKernelGGL(stem_pool_backward_kernel<T>, grid, block, 0, s, p);
            else hipLaunchKernelGGL(stem_pool_forward_kernel<T>, grid, block, 0, s, p);
        }
    });
}

}  // namespace mr

extern "C" int mr_stem_pool_forward(const void* x, const float* weight, const float* bias, const float* running_mean,
                                    const float* running_var, float eps, int act_dtype, int channels_last, void* y,
                                    unsigned char* argmax, int batch_size, int channels, int height, int width,
                                    mr_stream_t stream) {
    using namespace mr;
    if (act_dtype != 0 && act_dtype != 1) return MR_ERR_BADARG;
    if (channels_last && channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    StemParams p{};
    const int rc = stem_fill(p, x, weight, bias, running_mean, running_var, eps, batch_size, channels, height, width);
    if (rc != MR_OK) return rc;
    if (batch_size == 0 || channels == 0 || height == 0 || width == 0) return MR_OK;
    if (!x || !weight || !bias || !running_mean || !running_var || !y) return MR_ERR_BADARG;
    p.y = y;
    const int layout = stem_layout(channels_last);
    int64_t blocks = (int64_t)batch_size * channels * p.tiles_x * p.tiles_y;
    if (layout) {  // layout 2: argmax is the record buffer
        if (!stem_records_ok(argmax, layout) || !aligned4(x, act_dtype) || !aligned4(y, act_dtype)) return MR_ERR_BADARG;
        p.argmax = argmax;
        blocks = nhwc_blocks(stem_items(p, layout, false), channels, SP_NHWC_BLOCKS);
    }
    stem_launch<false>(p, act_dtype, layout, blocks, (hipStream_t)stream);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int64_t mr_stem_pool_records_bytes(int batch_size, int channels, int height, int width) {
    using namespace mr;
    StemParams p{};
    if (stem_fill(p, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f, batch_size, channels, height, width) != MR_OK) return -1;
    if (channels > 0 && !nhwc_channels_ok(channels)) return -1;
    const int64_t values = (int64_t)batch_size * p.OH * p.OW * channels;  // a multiple of 4
    return values * 4 + (values + 15) / 16 * 16;
}

extern "C" int64_t mr_stem_pool_backward_workspace_bytes(int batch_size, int channels, int height, int width) {
    using namespace mr;
    StemParams p{};
    if (stem_fill(p, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f, batch_size, channels, height, width) != MR_OK) return -1;
    return partial_bytes(2, channels, stem_slots(p, -1));
}

extern "C" int mr_stem_pool_backward(const void* grad_y, const void* grad_y2, const void* x, const unsigned char* argmax,
                                     const float* weight, const float* bias, const float* running_mean, const float* running_var, float eps,
                                     int act_dtype, int channels_last, void* grad_x, float* grad_weight,
                                     float* grad_bias, void* workspace, int64_t workspace_bytes, int batch_size,
                                     int channels, int height, int width, mr_stream_t stream) {
    using namespace mr;
    if (act_dtype != 0 && act_dtype != 1) return MR_ERR_BADARG;
    if (channels_last && channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    StemParams p{};
    const int rc = stem_fill(p, x, weight, bias, running_mean, running_var, eps, batch_size, channels, height, width);
    if (rc != MR_OK) return rc;
    if (channels == 0) return MR_OK;
    const bool want_params = grad_weight || grad_bias;
    if (batch_size == 0 || height == 0 || width == 0) return zero_param_grads({grad_weight, grad_bias}, channels, (hipStream_t)stream);
    const int layout = stem_layout(channels_last);
    if (!grad_y || (!x && layout != 2) || !weight || !bias || !running_mean || !running_var || !grad_x) return MR_ERR_BADARG;
    if (want_params &&
        (!workspace || workspace_bytes < mr_stem_pool_backward_workspace_bytes(batch_size, channels, height, width)))
        return MR_ERR_BADARG;
    p.grad_y = grad_y; p.grad_y2 = grad_y2; p.grad_x = grad_x;
    p.partial = want_params ? static_cast<float*>(workspace) : nullptr;
    if (layout) {  // layout 2, pooled records: x is not read and may be NULL (NULL counts as aligned)
        if (!stem_records_ok(argmax, layout) || (layout == 1 && !aligned4(x, act_dtype)) || !aligned4(grad_y, act_dtype) ||
            !aligned4(grad_y2, act_dtype) || !aligned4(grad_x, act_dtype))
            return MR_ERR_BADARG;
        p.argmax = const_cast<unsigned char*>(argmax);
    }
    const int64_t slots = stem_slots(p, layout);
    stem_launch<true>(p, act_dtype, layout, layout ? slots : slots * channels, (hipStream_t)stream);
    MR_CHECK_LAUNCH();
    if (!want_params) return MR_OK;
    return launch_bn_finish<2>(p.partial, slots, channels, bn_finish_out(running_var, eps, grad_weight, grad_bias), (hipStream_t)stream);
}

// grad_weight / grad_bias of the layout-2 backward alone (stem_pool_rec_sums_kernel): no x, no grad_x.  Workspace as for
// mr_stem_pool_backward; at least one of the two outputs must be asked for.
extern "C" int mr_stem_pool_param_grads(const void* grad_y, const void* grad_y2, const unsigned char* records, const float* weight,
                                        const float* bias, const float* running_mean, const float* running_var, float eps,
                                        int act_dtype, float* grad_weight, float* grad_bias, void* workspace,
                                        int64_t workspace_bytes, int batch_size, int channels, int height, int width,
                                        mr_stream_t stream) {
    using namespace mr;
    if (act_dtype != 0 && act_dtype != 1) return MR_ERR_BADARG;
    if (channels > 0 && !nhwc_channels_ok(channels)) return MR_ERR_BADARG;
    if (!grad_weight && !grad_bias) return MR_ERR_BADARG;
    StemParams p{};
    const int rc = stem_fill(p, nullptr, weight, bias, running_mean, running_var, eps, batch_size, channels, height, width);
    if (rc != MR_OK) return rc;
    if (channels == 0) return MR_OK;
    if (batch_size == 0 || height == 0 || width == 0) return zero_param_grads({grad_weight, grad_bias}, channels, (hipStream_t)stream);
    if (!grad_y || !weight || !bias || !running_mean || !running_var) return MR_ERR_BADARG;
    if (!workspace || workspace_bytes < mr_stem_pool_backward_workspace_bytes(batch_size, channels, height, width)) return MR_ERR_BADARG;
    if (!stem_records_ok(records, 2) || !aligned4(grad_y, act_dtype) || !aligned4(grad_y2, act_dtype)) return MR_ERR_BADARG;
    p.grad_y = grad_y; p.grad_y2 = grad_y2;
    p.partial = static_cast<float*>(workspace);
    p.argmax = const_cast<unsigned char*>(records);
    const int64_t slots = stem_slots(p, 2);
    const dim3 grid((unsigned)slots), block(256);
    dispatch_act(act_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(stem_pool_rec_sums_kernel<T>, grid, block, 0, (hipStream_t)stream, p);
    });
    MR_CHECK_LAUNCH();
    return launch_bn_finish<2>(p.partial, slots, channels, bn_finish_out(running_var, eps, grad_weight, grad_bias), (hipStream_t)stream);
}
