// frame_jpeg.hip -- JPEG frames on gfx950: the host stage's C-ABI (jpeg_entropy.hpp: parser + Huffman decoder -> one packed
// frame per file) and the device stage that turns N packed frames of one geometry into uint8 [N,H,W,3], byte for byte
// what Pillow (libjpeg-turbo, its defaults: islow IDCT, fancy upsampling) decodes.
//
//   jpeg_idct_kernel   one 8x8 block per thread, all 64 values in registers: 8 x 16-byte loads of the block's 128 contiguous
//                      bytes, dequantisation, libjpeg's jidctint (CONST_BITS 13, PASS1_BITS 2: columns first, descaled by
//                      11 bits, then rows, descaled by 18), range limit, eight 8-byte row stores into the component's u8
//                      plane (padded to whole MCUs) in the workspace.  int32 throughout; no LDS.
//                      Range limit: libjpeg's table look-up range_limit[x & 1023] -- as arithmetic: x taken as a signed
//                      10-bit number, plus 128, clamped to [0, 255]; a plain clamp differs once |x| passes 512.
//   jpeg_color_kernel  a thread owns 4 consecutive pixels of the [N,H,W,3] tensor (12 bytes: three whole dwords).  Chroma by
//                      libjpeg-turbo's fancy upsampling where the chroma plane is more than 2 samples wide (h2v1:
//                      (3 a + b + 1) >> 2 / (3 a + b + 2) >> 2; h2v2: the 3:1 vertical blend of two rows, then
//                      (3 a + b + 8) >> 4 / (3 a + b + 7) >> 4; first and last column a alone), plain replication below
//                      that; the rows above the first and below the last REAL chroma row (ceil(H v / vmax) rows) are those
//                      rows themselves.  Then jdcolor's SCALEBITS-16 tables as their defining expressions.  Grey frames
//                      replicate Y.
//
// Two launches per call whatever N; no float arithmetic -- the index divisions are multiplications by reciprocals the host
// prepares (the compiler would lower a runtime division through v_rcp_f32) --, no atomics, no copy: the tables ride in
// the packed frames.  The IDCT runs in 32-bit two's-complement arithmetic written on unsigned values (defined on overflow);
// the host stage only passes coefficients whose product with their quantiser fits 16 bits, and for every stream encoded
// from 8-bit samples all intermediate values stay far inside 32 bits, where libjpeg's 64-bit JLONG computes the same.
#include "jpeg_entropy.hpp"
#include "mr_common.hpp"

namespace mr {

constexpr int FJ_THREADS = 256;

struct JpegParams {
    const uint8_t* packed;  // [N] packed frames, frame_bytes apart
    uint8_t* planes;        // workspace: per frame the components' padded u8 planes, one after the other
    uint8_t* out;           // [N,H,W,3]
    int64_t frame_bytes;    // bytes of a packed frame
    int64_t plane_bytes;    // bytes of a frame's planes: 64 per block
    unsigned total_blocks;  // N * blocks
    unsigned total_pixels;  // N * H * W
    unsigned frame_pixels;  // H * W
    unsigned m_blocks, m_bw0, m_bwc, m_frame_pixels, m_W;  // reciprocals (udiv) of blocks, bw0, bwc, frame_pixels, W
    int blocks;             // blocks of a frame
    int base1, base2;       // first block of Cb, of Cr
    int bw0, bwc;           // blocks across the luma plane, across a chroma plane
    int N, H, W, ncomp;
    int mode;               // chroma: 0 full size, 1 h2v1, 2 h2v2
    int cw, ch;             // real samples across / down a chroma plane
};

// floor(2^32 / d) (d = 1: 2^32 - 1): the host's half of udiv
static inline unsigned udiv_magic(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)(((uint64_t)1 << 32) / d); }
// n / d for any 32-bit n: the high product is the quotient or one below it
__device__ __forceinline__ unsigned udiv(unsigned n, unsigned d, unsigned magic) {
    const unsigned q = __umulhi(n, magic);
    return n - q * d >= d ? q + 1 : q;
}

// One pass of jidctint.c over 8 values in place.  SHIFT: CONST_BITS - PASS1_BITS (columns), CONST_BITS + PASS1_BITS + 3 (rows).
template <int SHIFT>
__device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    typedef unsigned U;  // two's-complement arithmetic that is defined when it wraps; negative constants as their U image
    U z2 = (U)d2, z3 = (U)d6;
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 + z3 * (U)-15137;
    U tmp3 = z1 + z2 * 6270u;
    U tmp0 = ((U)d0 + (U)d4) * 8192u;
    U tmp1 = ((U)d0 - (U)d4) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)d7; tmp1 = (U)d5; tmp2 = (U)d3; tmp3 = (U)d1;
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (U)-7373; z2 *= (U)-20995; z3 *= (U)-16069; z4 *= (U)-3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr U R = 1u << (SHIFT - 1);
    d0 = (int)(tmp10 + tmp3 + R) >> SHIFT; d7 = (int)(tmp10 - tmp3 + R) >> SHIFT;
    d1 = (int)(tmp11 + tmp2 + R) >> SHIFT; d6 = (int)(tmp11 - tmp2 + R) >> SHIFT;
    d2 = (int)(tmp12 + tmp1 + R) >> SHIFT; d5 = (int)(tmp12 - tmp1 + R) >> SHIFT;
    d3 = (int)(tmp13 + tmp0 + R) >> SHIFT; d4 = (int)(tmp13 - tmp0 + R) >> SHIFT;
}

// range_limit[x & RANGE_MASK] of the IDCT (the table centred on 128)
__device__ __forceinline__ unsigned idct_limit(int x) {
    int s = (int)((unsigned)x << 22) >> 22;  // the low 10 bits, sign-extended
    s += 128;
    return (unsigned)(s < 0 ? 0 : s > 255 ? 255 : s);
}

__global__ __launch_bounds__(FJ_THREADS) void jpeg_idct_kernel(JpegParams p) {
    const unsigned gid = blockIdx.x * FJ_THREADS + threadIdx.x;
    if (gid >= p.total_blocks) return;
    const unsigned n = udiv(gid, (unsigned)p.blocks, p.m_blocks);
    const int j = (int)(gid - n * (unsigned)p.blocks);
    const int c = p.ncomp == 1 || j < p.base1 ? 0 : j < p.base2 ? 1 : 2;
    const int base = c == 0 ? 0 : c == 1 ? p.base1 : p.base2;
    const int bw = c == 0 ? p.bw0 : p.bwc;
    const int jb = j - base;
    const int by = (int)udiv((unsigned)jb, (unsigned)bw, c == 0 ? p.m_bw0 : p.m_bwc), bx = jb - by * bw;
    const uint8_t* frame = p.packed + (int64_t)n * p.frame_bytes;
    const int tq = reinterpret_cast<const int*>(frame)[6 + c] & 3;
    const uint4* qv = reinterpret_cast<const uint4*>(frame + 64 + 128 * tq);
    const uint4* cv = reinterpret_cast<const uint4*>(frame + mrjpeg::JE_HEADER_BYTES + (int64_t)j * 128);
    int v[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint4 cw = cv[r], qw = qv[r];
        const unsigned cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[r][2 * k] = ((int)(cs[k] << 16) >> 16) * (int)(qs[k] & 0xffffu);
            v[r][2 * k + 1] = ((int)cs[k] >> 16) * (int)(qs[k] >> 16);
        }
    }
#pragma unroll
    for (int x = 0; x < 8; x++) idct8<11>(v[0][x], v[1][x], v[2][x], v[3][x], v[4][x], v[5][x], v[6][x], v[7][x]);
    uint8_t* dst = p.planes + (int64_t)n * p.plane_bytes + (int64_t)base * 64 + ((int64_t)by * 8 * bw + bx) * 8;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        idct8<18>(v[r][0], v[r][1], v[r][2], v[r][3], v[r][4], v[r][5], v[r][6], v[r][7]);
        uint2 o;
        o.x = idct_limit(v[r][0]) | (idct_limit(v[r][1]) << 8) | (idct_limit(v[r][2]) << 16) | (idct_limit(v[r][3]) << 24);
        o.y = idct_limit(v[r][4]) | (idct_limit(v[r][5]) << 8) | (idct_limit(v[r][6]) << 16) | (idct_limit(v[r][7]) << 24);
        *reinterpret_cast<uint2*>(dst + (int64_t)r * bw * 8) = o;
    }
}

// a chroma sample at full resolution; `plane` is pw bytes wide, (cw, ch) of it are real samples
__device__ __forceinline__ int chroma_at(const uint8_t* plane, int pw, int cw, int ch, int mode, int x, int y) {
    if (mode == 0) return plane[(int64_t)y * pw + x];
    const int cx = x >> 1;
    if (mode == 1) {
        const uint8_t* row = plane + (int64_t)y * pw;
        const int a = row[cx];
        if (cw <= 2) return a;
        if (x & 1) return cx == cw - 1 ? a : (3 * a + row[cx + 1] + 2) >> 2;
        return cx == 0 ? a : (3 * a + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* row0 = plane + (int64_t)cy * pw;
    if (cw <= 2) return row0[cx];
    const int ny = (y & 1) ? (cy + 1 < ch ? cy + 1 : cy) : (cy > 0 ? cy - 1 : cy);
    const uint8_t* row1 = plane + (int64_t)ny * pw;
    const int a = 3 * row0[cx] + row1[cx];
    if (x & 1) return cx == cw - 1 ? (4 * a + 7) >> 4 : (3 * a + 3 * row0[cx + 1] + row1[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * a + 8) >> 4 : (3 * a + 3 * row0[cx - 1] + row1[cx - 1] + 8) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(FJ_THREADS) void jpeg_color_kernel(JpegParams p) {
    const unsigned group = blockIdx.x * FJ_THREADS + threadIdx.x;
    if (group >= (p.total_pixels + 3u) / 4u) return;  // (total_pixels <= 2^32 - 4)
    const unsigned p0 = group * 4u;
    unsigned n = udiv(p0, p.frame_pixels, p.m_frame_pixels);
    const unsigned rem = p0 - n * p.frame_pixels;
    int y = (int)udiv(rem, (unsigned)p.W, p.m_W);
    int x = (int)(rem - (unsigned)y * (unsigned)p.W);
    const int count = p.total_pixels - p0 < 4u ? (int)(p.total_pixels - p0) : 4;
    const int pw0 = p.bw0 * 8, pwc = p.bwc * 8;
    unsigned px[12];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        unsigned r = 0, g = 0, b = 0;
        if (i < count) {
            const uint8_t* planes = p.planes + (int64_t)n * p.plane_bytes;
            const int Y = planes[(int64_t)y * pw0 + x];
            if (p.ncomp == 1) {
                r = g = b = (unsigned)Y;
            } else {
                const int cb = chroma_at(planes + (int64_t)p.base1 * 64, pwc, p.cw, p.ch, p.mode, x, y) - 128;
                const int cr = chroma_at(planes + (int64_t)p.base2 * 64, pwc, p.cw, p.ch, p.mode, x, y) - 128;
                // jdcolor.c build_ycc_rgb_table: FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414) at SCALEBITS 16
                r = clamp255(Y + ((91881 * cr + 32768) >> 16));
                g = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                b = clamp255(Y + ((116130 * cb + 32768) >> 16));
            }
            if (++x == p.W) {
                x = 0;
                if (++y == p.H) {
                    y = 0;
                    n++;
                }
            }
        }
        px[3 * i] = r; px[3 * i + 1] = g; px[3 * i + 2] = b;
    }
    uint8_t* dst = p.out + (int64_t)p0 * 3;
    if (count == 4) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        d[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        d[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        d[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
    } else {
        for (int k = 0; k < 3 * count; k++) dst[k] = (uint8_t)px[k];
    }
}

}  // namespace mr

extern "C" int mr_jpeg_info(const unsigned char* data, int64_t len, int* info) {
    if (!data || !info || len < 0) return MR_ERR_BADARG;
    mrjpeg::JeStream s;
    const int rc = mrjpeg::je_parse(data, len, s);
    if (rc != mrjpeg::JE_OK) return rc;
    info[0] = s.g.width; info[1] = s.g.height; info[2] = s.g.ncomp; info[3] = s.g.hl; info[4] = s.g.vl; info[5] = s.restart;
    return MR_OK;
}

extern "C" int64_t mr_jpeg_packed_bytes(int width, int height, int components, int luma_h, int luma_v) {
    return mrjpeg::je_packed_bytes(width, height, components, luma_h, luma_v);
}

extern "C" int mr_jpeg_entropy_decode(const unsigned char* data, int64_t len, unsigned char* packed, int64_t packed_bytes) {
    if (!data || !packed || len < 0 || mr::misaligned({packed}, 3)) return MR_ERR_BADARG;
    mrjpeg::JeStream s;
    const int rc = mrjpeg::je_parse(data, len, s);
    if (rc != mrjpeg::JE_OK) return rc;
    return mrjpeg::je_decode(data, len, s, packed, packed_bytes);
}

// workspace: ONE region at the base, the frames' planes after the IDCT, 64 bytes per block
static int64_t jpeg_work_bytes(int num_frames, const mrjpeg::JeGeometry& g) { return (int64_t)num_frames * 64 * g.blocks; }

extern "C" int64_t mr_jpeg_reconstruct_workspace_bytes(int num_frames, int width, int height, int components, int luma_h,
                                                       int luma_v) {
    mrjpeg::JeGeometry g;
    if (num_frames < 0 || !mrjpeg::je_geometry(width, height, components, luma_h, luma_v, g)) return -1;
    return jpeg_work_bytes(num_frames, g);
}

extern "C" int mr_jpeg_reconstruct(const unsigned char* packed, int num_frames, int width, int height, int components,
                                   int luma_h, int luma_v, unsigned char* frames_out, void* workspace, int64_t workspace_bytes,
                                   mr_stream_t stream) {
    using namespace mr;
    mrjpeg::JeGeometry g;
    if (num_frames < 0 || !mrjpeg::je_geometry(width, height, components, luma_h, luma_v, g)) return MR_ERR_BADARG;
    if (num_frames == 0) return MR_OK;
    if (!packed || !frames_out || !workspace) return MR_ERR_BADARG;
    if (misaligned({packed, workspace}, 15) || misaligned({frames_out}, 3)) return MR_ERR_BADARG;
    if (workspace_bytes < jpeg_work_bytes(num_frames, g)) return MR_ERR_BADARG;
    JpegParams p{};
    p.packed = packed;
    p.planes = static_cast<uint8_t*>(workspace);
    p.out = frames_out;
    p.frame_bytes = mrjpeg::JE_HEADER_BYTES + 128 * g.blocks;
    p.plane_bytes = 64 * g.blocks;
    // a thread's pixel and block numbers are 32-bit: up to 2^32 - 4 pixels (12.9 GB of frames) and blocks in one call
    const int64_t total_blocks = (int64_t)num_frames * g.blocks, total_pixels = (int64_t)num_frames * height * width;
    if (total_pixels > 0xfffffffcll || total_blocks > 0xfffffe00ll) return MR_ERR_NOTIMPL;  // (+ a workgroup: no wrap)
    p.total_blocks = (unsigned)total_blocks;
    p.total_pixels = (unsigned)total_pixels;
    p.frame_pixels = (unsigned)(height * width);
    p.blocks = (int)g.blocks;
    p.base1 = (int)g.block_base[1]; p.base2 = (int)g.block_base[2];
    p.bw0 = g.bw[0]; p.bwc = g.bw[1];
    p.m_blocks = udiv_magic((unsigned)p.blocks); p.m_bw0 = udiv_magic((unsigned)p.bw0); p.m_bwc = udiv_magic((unsigned)p.bwc);
    p.m_frame_pixels = udiv_magic(p.frame_pixels); p.m_W = udiv_magic((unsigned)width);
    p.N = num_frames; p.H = height; p.W = width; p.ncomp = components;
    p.mode = luma_h == 1 ? 0 : luma_v == 1 ? 1 : 2;
    p.cw = (width + luma_h - 1) / luma_h;
    p.ch = (height + luma_v - 1) / luma_v;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total_blocks + FJ_THREADS - 1) / FJ_THREADS)), dim3(FJ_THREADS), 0, s, p);
    MR_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((total_pixels + FJ_THREADS * 4 - 1) / (FJ_THREADS * 4))),
                       dim3(FJ_THREADS), 0, s, p);
    MR_CHECK_LAUNCH();
    return MR_OK;
}
