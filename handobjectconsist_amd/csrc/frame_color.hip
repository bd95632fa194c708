// frame_color.hip -- colour augmentation of decoded frames on gfx950: the device counterpart of datasets/coloraugm.py
// (PIL ImageFilter.GaussianBlur, then ImageEnhance Brightness / Color / Contrast and the hue shift in a per-frame order),
// for a whole batch of frames, byte for byte what Pillow computes.
//
//   GaussianBlur   three box passes along the rows, three along the columns, every pass rounded to u8 (BoxBlur.c):
//                  out[x] = (ww * sum_{|k| <= rad} in[clamp(x + k)] + fw * (in[clamp(x - rad - 1)] + in[clamp(x + rad + 1)])
//                            + 2^23) >> 24 in 32-bit unsigned arithmetic; rad, ww, fw from the radius in float32 (host side,
//                  the very operations Pillow's C performs).
//   enhance ops    blend(degenerate, image, f): t = d + f * (i - d) in float32, truncated for 0 <= f <= 1, else clipped
//                  (Blend.c); d = 0 (brightness), L (saturation), int(mean(L) + 0.5) of the whole frame (contrast);
//                  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
//   hue            RGB -> HSV, H += shift (mod 256), HSV -> RGB with Convert.c's mix of float variables and double literals.
//
// Launches: the plans (kernel arguments -> workspace, 64 frames per launch), the row passes (frames -> workspace copy), the
// column passes + every op in front of the frame's contrast op + the exact integer sum of L where a contrast op follows
// (workspace copy -> output), and -- only if some frame has a contrast op -- contrast and what follows it, in place on the
// output.  A line is blurred in LDS: every thread owns runs of FC_SEG outputs, starts each from an exact clamped window sum
// and slides it (two LDS reads per output whatever the radius); integer arithmetic, so the result does not depend on
// how a line is cut.  No float atomics; the L sums are 64-bit integer atomics (order-independent).
//
// Mirrored samples (handobjset.py: mirror, augment, mirror back): every stage is mirror-symmetric -- the clamped window and
// its two fractional taps are symmetric sums of integers, the ops look at one pixel and at the frame's sum -- so the flip
// flag changes nothing here; tests/test_oracle_coloraugm.py and the Pillow fixture hold flipped cases.
#include <math.h>

#include <vector>

#include "mr_common.hpp"

namespace mr {

struct __attribute__((aligned(8))) ColorPlan {
    int blur;          // 0: the frame is copied (radius 0)
    int rad;           // integer box radius of a pass
    unsigned ww, fw;   // 8.24 weights of a full tap and of the two fractional taps
    int nops;          // ops in application order, MR_COLOR_OP_NONE entries removed
    int split;         // index of the contrast op (nops if there is none): ops [0, split) need no whole-frame value
    unsigned char code[4];
    float value[4];    // blend factor; hue: the integer shift of the H byte
    int pad;
};

constexpr int FC_PLANS_PER_LAUNCH = 64;
struct ColorPlanBlock {
    ColorPlan plan[FC_PLANS_PER_LAUNCH];
};

struct ColorParams {
    const uint8_t* in;         // [N,Hs,Ws,3]
    uint8_t* tmp;              // [N,Hs,Ws,3] row-blurred frames (workspace)
    uint8_t* out;              // [N,Hs,Ws,3]
    ColorPlan* plans;          // [N]
    unsigned long long* lsum;  // [N] sum of L over the frame where its contrast op stands
    int N, Hs, Ws;
    int rows_per_block;        // row kernel: rows of a workgroup
    int strip_px;              // column kernel: pixels across a workgroup's strip
};

constexpr int FC_THREADS = 256;
constexpr int FC_SEG = 16;          // outputs of a run
constexpr int FC_LDS = 32256;       // bytes of one of the two line buffers (63 KB of LDS together: two workgroups per CU)
constexpr int FC_MAX_DIM = FC_LDS / 3;  // longest line (pixels) a workgroup can hold: 10752

__global__ __launch_bounds__(FC_PLANS_PER_LAUNCH) void color_plans_kernel(ColorPlanBlock blk, ColorPlan* plans,
                                                                         unsigned long long* lsum, int first, int count) {
    const int k = threadIdx.x;
    if (k >= count) return;
    plans[first + k] = blk.plan[k];
    lsum[first + k] = 0ull;
}

// One run of a box pass: outputs [x0, x1) of a line of n samples `stride` bytes apart.
__device__ __forceinline__ void box_run(const uint8_t* in, uint8_t* out, int n, int stride, int x0, int x1, int rad, unsigned ww,
                                        unsigned fw) {
    const int lo = x0 - rad, hi = x0 + rad;
    const int clo = max(lo, 0), chi = min(hi, n - 1);
    unsigned acc = (unsigned)(clo - lo) * in[0] + (unsigned)(hi - chi) * in[(size_t)(n - 1) * stride];  // taps beyond the edges
    for (int k = clo; k <= chi; k++) acc += in[(size_t)k * stride];
    unsigned a = in[(size_t)min(max(x0 - rad - 1, 0), n - 1) * stride];
    for (int x = x0; x < x1; x++) {
        const unsigned b = in[(size_t)min(x + rad + 1, n - 1) * stride];
        out[(size_t)x * stride] = (uint8_t)((acc * ww + (a + b) * fw + (1u << 23)) >> 24);
        a = in[(size_t)min(max(x - rad, 0), n - 1) * stride];
        acc += b - a;  // window of x + 1
    }
}

// `rows` lines of `bytes` bytes between global memory (pitch gpitch) and LDS (pitch lpitch); dwords where everything is aligned
template <bool TO_LDS>
__device__ __forceinline__ void move_lines(uint8_t* g, size_t gpitch, uint8_t* l, int lpitch, int rows, int bytes) {
    const int tid = threadIdx.x;
    if ((((uintptr_t)g | gpitch | (unsigned)lpitch | (unsigned)bytes) & 3) == 0) {
        const int dw = bytes >> 2;
        for (int e = tid; e < rows * dw; e += FC_THREADS) {
            const int r = e / dw, c = e - r * dw;
            unsigned* gp = reinterpret_cast<unsigned*>(g + (size_t)r * gpitch) + c;
            unsigned* lp = reinterpret_cast<unsigned*>(l + (size_t)r * lpitch) + c;
            if (TO_LDS) *lp = *gp;
            else *gp = *lp;
        }
    } else {
        for (int e = tid; e < rows * bytes; e += FC_THREADS) {
            const int r = e / bytes, c = e - r * bytes;
            if (TO_LDS) l[(size_t)r * lpitch + c] = g[(size_t)r * gpitch + c];
            else g[(size_t)r * gpitch + c] = l[(size_t)r * lpitch + c];
        }
    }
}

// ---- the per-pixel ops ----
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int blend1(int d, int i, float f) {
    const float t = (float)d + f * (float)(i - d);
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ void hue_shift(int shift, int& r, int& g, int& b) {
    // rgb2hsv_row
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double t = (double)h / 6.0 + 1.0;  // in [5/6, 11/6]: fmod(t, 1) = t - floor(t), exact
        h = (float)(t - floor(t));
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    // hsv2rgb
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double h6 = (double)uh * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const double f = (double)(float)(h6 - (double)i);
    const double fs = (double)(float)((double)us / 255.0);
    const double v = (double)uv;
    const int p = clip8((int)round(v * (1.0 - fs)));
    const int q = clip8((int)round(v * (1.0 - fs * f)));
    const int t = clip8((int)round(v * (1.0 - fs * (1.0 - f))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// ops [first, last) of a plan on one pixel; `mean`: the grey level of the frame's contrast op
__device__ __forceinline__ void color_ops(const ColorPlan& pl, int first, int last, int mean, int& r, int& g, int& b) {
    for (int k = first; k < last; k++) {
        const int code = pl.code[k];  // (the same for every pixel of a frame: no divergence)
        const float f = pl.value[k];
        if (code == MR_COLOR_OP_HUE) {
            hue_shift((int)f, r, g, b);
        } else {
            const int l = luma(r, g, b);
            const int dr = code == MR_COLOR_OP_BRIGHTNESS ? 0 : (code == MR_COLOR_OP_SATURATION ? l : mean);
            r = blend1(dr, r, f);
            g = blend1(dr, g, f);
            b = blend1(dr, b, f);
        }
    }
}

// grid (ceil(Hs / rows_per_block), N): rows_per_block whole rows in LDS, three passes along them, into the workspace copy
__global__ __launch_bounds__(FC_THREADS) void color_blur_rows_kernel(ColorParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[2][FC_LDS];
    const int n = blockIdx.y, r0 = blockIdx.x * p.rows_per_block;
    const int nr = min(p.rows_per_block, p.Hs - r0);
    const int rowbytes = p.Ws * 3;
    const size_t off = ((size_t)n * p.Hs + r0) * rowbytes;
    const ColorPlan pl = p.plans[n];
    move_lines<true>(const_cast<uint8_t*>(p.in) + off, rowbytes, buf[0], rowbytes, nr, rowbytes);
    __syncthreads();
    int cur = 0;
    if (pl.blur) {
        const int nseg = (p.Ws + FC_SEG - 1) / FC_SEG;
        for (int pass = 0; pass < 3; pass++) {
            for (int it = threadIdx.x; it < nr * nseg * 3; it += FC_THREADS) {
                const int c = it % 3, s = (it / 3) % nseg, r = it / (3 * nseg);
                box_run(buf[cur] + r * rowbytes + c, buf[cur ^ 1] + r * rowbytes + c, p.Ws, 3, s * FC_SEG,
                        min(p.Ws, (s + 1) * FC_SEG), pl.rad, pl.ww, pl.fw);
            }
            cur ^= 1;
            __syncthreads();
        }
    }
    move_lines<false>(p.tmp + off, rowbytes, buf[cur], rowbytes, nr, rowbytes);
}

// grid (ceil(Ws / strip_px), N): a strip of strip_px pixels x all Hs rows in LDS, three passes along the columns, then the
// ops in front of the frame's contrast op and the strip's share of the frame's L sum, into the output
__global__ __launch_bounds__(FC_THREADS) void color_blur_cols_kernel(ColorParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[2][FC_LDS];
    __shared__ unsigned block_sum;
    const int n = blockIdx.y, x0 = blockIdx.x * p.strip_px;
    const int sp = min(p.strip_px, p.Ws - x0), sb = sp * 3, pitch = p.strip_px * 3;
    const size_t rowbytes = (size_t)p.Ws * 3;
    const size_t off = (size_t)n * p.Hs * rowbytes + (size_t)x0 * 3;
    __shared__ ColorPlan pl;  // (indexed by the op loop: one copy in LDS, not one per thread)
    if (threadIdx.x == 0) {
        block_sum = 0u;
        pl = p.plans[n];
    }
    move_lines<true>(p.tmp + off, rowbytes, buf[0], pitch, p.Hs, sb);
    __syncthreads();
    int cur = 0;
    if (pl.blur) {
        const int nseg = (p.Hs + FC_SEG - 1) / FC_SEG;
        for (int pass = 0; pass < 3; pass++) {
            for (int it = threadIdx.x; it < nseg * sb; it += FC_THREADS) {
                const int c = it % sb, s = it / sb;
                box_run(buf[cur] + c, buf[cur ^ 1] + c, p.Hs, pitch, s * FC_SEG, min(p.Hs, (s + 1) * FC_SEG), pl.rad, pl.ww,
                        pl.fw);
            }
            cur ^= 1;
            __syncthreads();
        }
    }
    const bool contrast = pl.split < pl.nops;
    if (pl.split > 0 || contrast) {
        unsigned lsum = 0u;  // (a workgroup holds at most FC_LDS / 3 pixels: below 2^32)
        uint8_t* px = buf[cur];
        for (int it = threadIdx.x; it < p.Hs * sp; it += FC_THREADS) {
            const int y = it / sp, x = it - y * sp;
            uint8_t* q = px + y * pitch + 3 * x;
            int r = q[0], g = q[1], b = q[2];
            color_ops(pl, 0, pl.split, 0, r, g, b);
            q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b;
            lsum += (unsigned)luma(r, g, b);
        }
        if (contrast) atomicAdd(&block_sum, lsum);
        __syncthreads();
        if (contrast && threadIdx.x == 0) atomicAdd(&p.lsum[n], (unsigned long long)block_sum);
    }
    move_lines<false>(p.out + off, rowbytes, buf[cur], pitch, p.Hs, sb);
}

// grid (blocks, N): the contrast op and the ops behind it, in place on the output; frames without a contrast op are done
__global__ __launch_bounds__(FC_THREADS) void color_tail_kernel(ColorParams p) {
    const int n = blockIdx.y;
    __shared__ ColorPlan pl;
    if (threadIdx.x == 0) pl = p.plans[n];
    __syncthreads();
    if (pl.split >= pl.nops) return;
    const size_t pixels = (size_t)p.Hs * p.Ws;
    const int mean = (int)((double)p.lsum[n] / (double)pixels + 0.5);
    uint8_t* frame = p.out + (size_t)n * pixels * 3;
    for (size_t i = (size_t)blockIdx.x * FC_THREADS + threadIdx.x; i < pixels; i += (size_t)gridDim.x * FC_THREADS) {
        uint8_t* q = frame + 3 * i;
        int r = q[0], g = q[1], b = q[2];
        color_ops(pl, pl.split, pl.nops, mean, r, g, b);
        q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b;
    }
}

// workspace: the frames' plans | their luma sums | the row-blurred frames: places them in `p`, returns the bytes
static int64_t color_work(void* ws, int64_t n, int src_height, int src_width, ColorParams& p) {
    Carve c;
    p.plans = at_offset<ColorPlan>(ws, c.take(n * (int64_t)sizeof(ColorPlan)));
    p.lsum = at_offset<unsigned long long>(ws, c.take(n * 8));
    p.tmp = at_offset<uint8_t>(ws, c.take(n * src_height * src_width * 3));
    return c.total();
}

// Pillow's _gaussian_blur_radius + the weights of ImagingHorizontalBoxBlur: float variables, float32 operations
static void box_weights(float radius, ColorPlan& pl) {
    const float s2 = radius * radius / 3.0f;
    const float L = sqrtf(12.0f * s2 + 1.0f);
    const float l = floorf((L - 1.0f) / 2.0f);
    float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * s2);
    a = a / (6.0f * (s2 - (l + 1.0f) * (l + 1.0f)));
    const float fr = l + a;
    pl.rad = (int)fr;
    pl.ww = (unsigned)((float)(1 << 24) / (fr * 2.0f + 1.0f));
    pl.fw = ((1u << 24) - (unsigned)(pl.rad * 2 + 1) * pl.ww) / 2u;
}

}  // namespace mr

extern "C" int64_t mr_frames_color_augment_workspace_bytes(int num_frames, int src_height, int src_width) {
    if (num_frames < 0 || src_height < 0 || src_width < 0) return -1;
    mr::ColorParams p;
    return mr::color_work(nullptr, num_frames, src_height, src_width, p);
}

extern "C" int mr_frames_color_augment(const uint8_t* frames_in, uint8_t* frames_out, const uint8_t* flip,
                                       const float* blur_radius, const int* op_codes, const float* op_values, void* workspace,
                                       int64_t workspace_bytes, int num_frames, int src_height, int src_width,
                                       mr_stream_t stream) {
    using namespace mr;
    (void)flip;  // every stage is mirror-symmetric (see the head of this file)
    if (num_frames < 0 || src_height < 0 || src_width < 0) return MR_ERR_BADARG;
    if (num_frames == 0 || src_height == 0 || src_width == 0) return MR_OK;
    if (!frames_in || !frames_out || !blur_radius || !op_codes || !op_values || !workspace) return MR_ERR_BADARG;
    if (misaligned({frames_in, frames_out}, 3) || misaligned({workspace}, 15)) return MR_ERR_BADARG;
    ColorParams p{};  // (padding bytes are kernel-argument bytes too)
    if (workspace_bytes < color_work(workspace, num_frames, src_height, src_width, p)) return MR_ERR_BADARG;
    if (num_frames > 65535) return MR_ERR_NOTIMPL;  // a frame is a grid row (gridDim.y)
    std::vector<ColorPlan> plans((size_t)num_frames);
    bool any_contrast = false;
    for (int n = 0; n < num_frames; n++) {
        ColorPlan& pl = plans[(size_t)n];
        pl = ColorPlan();
        const float radius = blur_radius[n];
        if (!(radius >= 0.0f && radius <= 1024.0f)) return MR_ERR_BADARG;  // (also NaN)
        pl.blur = radius != 0.0f;
        if (pl.blur) box_weights(radius, pl);
        unsigned seen = 0;
        for (int k = 0; k < 4; k++) {
            const int code = op_codes[4 * n + k];
            const float v = op_values[4 * n + k];
            if (code == MR_COLOR_OP_NONE) continue;
            if (code != MR_COLOR_OP_BRIGHTNESS && code != MR_COLOR_OP_SATURATION && code != MR_COLOR_OP_HUE &&
                code != MR_COLOR_OP_CONTRAST)
                return MR_ERR_BADARG;
            if (seen & (1u << code)) return MR_ERR_BADARG;  // an op at most once (one frame mean per plan)
            seen |= 1u << code;
            if (!isfinite(v)) return MR_ERR_BADARG;
            if (code == MR_COLOR_OP_HUE && !(v >= -127.0f && v <= 127.0f && v == (float)(int)v)) return MR_ERR_BADARG;
            pl.code[pl.nops] = (unsigned char)code;
            pl.value[pl.nops] = v;
            pl.nops++;
        }
        pl.split = pl.nops;
        for (int k = 0; k < pl.nops; k++)
            if (pl.code[k] == MR_COLOR_OP_CONTRAST) pl.split = k;
        any_contrast = any_contrast || pl.split < pl.nops;
    }
    if (src_height > FC_MAX_DIM || src_width > FC_MAX_DIM) return MR_ERR_NOTIMPL;  // a line no longer fits a workgroup's LDS
    p.in = frames_in; p.out = frames_out;
    p.N = num_frames; p.Hs = src_height; p.Ws = src_width;
    p.rows_per_block = FC_LDS / (src_width * 3);
    if (p.rows_per_block > 16) p.rows_per_block = 16;
    p.strip_px = FC_LDS / (src_height * 3);
    if (p.strip_px > src_width) p.strip_px = src_width;
    if (p.strip_px >= 4) p.strip_px &= ~3;  // strips start on dword boundaries
    const hipStream_t s = (hipStream_t)stream;
    for (int first = 0; first < num_frames; first += FC_PLANS_PER_LAUNCH) {
        ColorPlanBlock blk;
        const int count = num_frames - first < FC_PLANS_PER_LAUNCH ? num_frames - first : FC_PLANS_PER_LAUNCH;
        for (int k = 0; k < FC_PLANS_PER_LAUNCH; k++) blk.plan[k] = plans[(size_t)(first + (k < count ? k : 0))];
        hipLaunchKernelGGL(color_plans_kernel, dim3(1), dim3(FC_PLANS_PER_LAUNCH), 0, s, blk, p.plans, p.lsum, first, count);
        MR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(color_blur_rows_kernel, dim3((unsigned)((src_height + p.rows_per_block - 1) / p.rows_per_block), (unsigned)num_frames),
                       dim3(FC_THREADS), 0, s, p);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(color_blur_cols_kernel, dim3((unsigned)((src_width + p.strip_px - 1) / p.strip_px), (unsigned)num_frames),
                       dim3(FC_THREADS), 0, s, p);
    MR_CHECK_LAUNCH();
    if (any_contrast) {
        const int64_t pixels = (int64_t)src_height * src_width;
        int64_t blocks = (pixels + FC_THREADS * 4 - 1) / (FC_THREADS * 4);
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(color_tail_kernel, dim3((unsigned)blocks, (unsigned)num_frames), dim3(FC_THREADS), 0, s, p);
        MR_CHECK_LAUNCH();
    }
    return MR_OK;
}
