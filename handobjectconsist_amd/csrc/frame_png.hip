// frame_png.hip -- PNG frames on gfx950, the device stage: N packed frames of one geometry (the filtered scanlines exactly as
// zlib inflated them on the host, datasets/pngdecode.py) -> uint8 [N,H,W,3], byte for byte what Pillow's
// Image.open(...).convert("RGB") gives: the PNG specification's five row filters undone (Recon = Filt + pred(a, b, c) mod 256;
// a = the byte bpp to the left, b = above, c = above-left, 0 outside the image), alpha dropped, grey replicated.
//
//   png_unfilter_kernel<BPP>  ONE WAVE (a workgroup of 64 threads) owns a frame and walks it in bands of MR_PNG_BAND_ROWS = 64
//       rows; lane l owns row band * 64 + l.  A step is a GROUP of 4 pixels (4 BPP bytes: BPP dwords): at step s lane l does
//       group s - l of its row, so the rows run as a skewed wavefront, each one group behind the row above -- what a group
//       needs of the row above (its 4 pixels, and the pixel left of them) is what the lane above produced one and two steps
//       earlier.  It travels as BPP dwords through one DPP wave shift per dword (wave_shr:1); the last row of a band is
//       written to an LDS line (4 BPP ceil(W / 4) bytes) that lane 0 of the next band reads: the same wave, so program order
//       is the only synchronisation needed -- a workgroup barrier separates the bands all the same.  No workgroup waits for
//       another; there is no flag and no atomic.
//       A lane reads its row through aligned dwords only -- rows are 1 + W BPP bytes apart, so v_alignbyte realigns them by
//       the row's own offset; BPP new dwords per step, loaded one step ahead -- and takes its filter byte once per band.
//       Every loop bound (bands, steps) is a number the host computed from width and height.  The filter is applied
//       branch-free (all five predictors are a handful of integer operations; a lane's filter is a select), so the DPP
//       shifts always run with the whole wave active.  Unknown filter bytes (the host refuses them) act as filter 0.
//       Output: where W is a multiple of 4 every group is three whole, aligned dwords of the [N,H,W,3] tensor; other widths
//       (rows that start at odd bytes) store bytes.
//
// One launch per call whatever N; no workspace, no scratch, no float instruction.
#include "mr_common.hpp"

namespace mr {

constexpr int PNG_BAND = MR_PNG_BAND_ROWS;
static_assert(PNG_BAND == MR_WAVE, "a band is one row per lane of a wave");

struct PngParams {
    const uint8_t* packed;  // [N] packed frames, frame_bytes apart
    uint8_t* out;           // [N,H,W,3]
    int64_t frame_bytes;    // bytes of a packed frame (a multiple of 16)
    int H, W;
    int stride;             // bytes of a filtered scanline: 1 + W * BPP
    int groups;             // ceil(W / 4)
    int bands;              // ceil(H / 64)
    int steps;              // steps of a band: groups + 63
    int last_dword;         // index of the frame's last dword
    int dword_stores;       // W % 4 == 0: a group is three aligned dwords of the output
};

__device__ __forceinline__ unsigned wave_shr1(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);  // wave_shr:1 (lane 0 keeps the 0)
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

template <int BPP>
__global__ __launch_bounds__(MR_WAVE) void png_unfilter_kernel(PngParams p) {
    extern __shared__ unsigned png_line[];  // [groups * BPP] dwords: the reconstructed last row of the previous band
    const int lane = threadIdx.x;
    const uint8_t* frame = p.packed + (int64_t)blockIdx.x * p.frame_bytes;
    const unsigned* fw = reinterpret_cast<const unsigned*>(frame);
    uint8_t* out_frame = p.out + (int64_t)blockIdx.x * p.H * p.W * 3;

    for (int band = 0; band < p.bands; band++) {
        const int y = band * PNG_BAND + lane;
        const bool row = y < p.H;
        const int o = MR_PNG_HEADER_BYTES + (row ? y : 0) * p.stride + 1;  // the row's first data byte
        const int q = o >> 2;
        const unsigned sh = (unsigned)o & 3u;
        const int ft = row ? frame[o - 1] : 0;
        uint8_t* out_row = out_frame + (int64_t)(row ? y : 0) * p.W * 3;

        unsigned carry = 0;           // the last dword loaded: the next group's first
        unsigned nxt[BPP];            // the dwords loaded for the NEXT step
        unsigned cur[BPP];            // this lane's reconstructed group of the last step
        int left[BPP], upleft[BPP];   // the pixel left of the group: this row's, the row above's
#pragma unroll
        for (int j = 0; j < BPP; j++) nxt[j] = cur[j] = 0, left[j] = upleft[j] = 0;
        if (row && lane == 0) {  // (group 0 of lane 0 is step 0: its dwords are loaded here)
            carry = fw[q];
#pragma unroll
            for (int j = 0; j < BPP; j++) nxt[j] = fw[min(q + 1 + j, p.last_dword)];
        }

        for (int s = 0; s < p.steps; s++) {
            const int g = s - lane;
            const bool active = row && g >= 0 && g < p.groups;
            // the row above: the lane above's last group (all lanes active here), lane 0's from the band before
            unsigned up[BPP];
#pragma unroll
            for (int j = 0; j < BPP; j++) up[j] = wave_shr1(cur[j]);
            if (lane == 0 && band > 0 && active) {
#pragma unroll
                for (int j = 0; j < BPP; j++) up[j] = png_line[g * BPP + j];
            }
            // this group's filtered bytes, realigned; then the loads of the next step
            unsigned win[BPP + 1];
            win[0] = carry;
#pragma unroll
            for (int j = 0; j < BPP; j++) win[j + 1] = nxt[j];
            carry = win[BPP];
            const int gn = g + 1;
            if (row && gn >= 0 && gn < p.groups) {
                if (gn == 0) carry = fw[q];
#pragma unroll
                for (int j = 0; j < BPP; j++) nxt[j] = fw[min(q + gn * BPP + 1 + j, p.last_dword)];
            }
            unsigned in[BPP];
#pragma unroll
            for (int j = 0; j < BPP; j++) in[j] = __builtin_amdgcn_alignbyte(win[j + 1], win[j], sh);
            if (g <= 0) {
#pragma unroll
                for (int j = 0; j < BPP; j++) left[j] = upleft[j] = 0;
            }
            int R[4 * BPP];
#pragma unroll
            for (int i = 0; i < 4 * BPP; i++) {
                const int f = (int)((in[i >> 2] >> (8 * (i & 3))) & 255u);
                const int b = (int)((up[i >> 2] >> (8 * (i & 3))) & 255u);
                const int a = i < BPP ? left[i % BPP] : R[i >= BPP ? i - BPP : 0];
                const int c = i < BPP ? upleft[i % BPP] : (int)((up[(i >= BPP ? i - BPP : 0) >> 2] >> (8 * ((i >= BPP ? i - BPP : 0) & 3))) & 255u);
                const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth(a, b, c) : 0;
                R[i] = (f + pred) & 255;
            }
#pragma unroll
            for (int j = 0; j < BPP; j++) {
                left[j] = R[3 * BPP + j];
                upleft[j] = (int)((up[(3 * BPP + j) >> 2] >> (8 * ((3 * BPP + j) & 3))) & 255u);
                cur[j] = (unsigned)R[4 * j] | ((unsigned)R[4 * j + 1] << 8) | ((unsigned)R[4 * j + 2] << 16) | ((unsigned)R[4 * j + 3] << 24);
            }
            if (active) {
                if (lane == PNG_BAND - 1) {
#pragma unroll
                    for (int j = 0; j < BPP; j++) png_line[g * BPP + j] = cur[j];
                }
                unsigned px[12];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    px[3 * k] = (unsigned)R[k * BPP];
                    px[3 * k + 1] = (unsigned)R[k * BPP + (BPP >= 3 ? 1 : 0)];
                    px[3 * k + 2] = (unsigned)R[k * BPP + (BPP >= 3 ? 2 : 0)];
                }
                uint8_t* dst = out_row + (int64_t)g * 12;
                if (p.dword_stores) {
                    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
                    d[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
                    d[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
                    d[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
                } else {
                    const int count = min(4, p.W - 4 * g);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (k < count) {
                            dst[3 * k] = (uint8_t)px[3 * k];
                            dst[3 * k + 1] = (uint8_t)px[3 * k + 1];
                            dst[3 * k + 2] = (uint8_t)px[3 * k + 2];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

static inline bool png_geometry_ok(int width, int height, int channels) {
    return width >= 1 && height >= 1 && channels >= 1 && channels <= 4;
}

}  // namespace mr

extern "C" int64_t mr_png_packed_bytes(int width, int height, int channels) {
    if (!mr::png_geometry_ok(width, height, channels) || width > MR_PNG_MAX_SIDE || height > MR_PNG_MAX_SIDE) return -1;
    return (MR_PNG_HEADER_BYTES + (int64_t)height * (1 + (int64_t)width * channels) + 15) & ~(int64_t)15;
}

extern "C" int64_t mr_png_unfilter_workspace_bytes(int num_frames, int width, int height, int channels) {
    if (num_frames < 0 || mr_png_packed_bytes(width, height, channels) < 0) return -1;
    return 0;
}

extern "C" int mr_png_unfilter(const unsigned char* packed, int num_frames, int width, int height, int channels,
                               unsigned char* frames_out, void* workspace, mr_stream_t stream) {
    using namespace mr;
    (void)workspace;  // (none is needed: mr_png_unfilter_workspace_bytes is 0)
    if (num_frames < 0 || !png_geometry_ok(width, height, channels)) return MR_ERR_BADARG;
    if (num_frames == 0) return MR_OK;
    if (!packed || !frames_out) return MR_ERR_BADARG;
    if (misaligned({packed}, 15) || misaligned({frames_out}, 3)) return MR_ERR_BADARG;
    // a frame's byte offsets are 32-bit and a reconstructed row lives in LDS: 4 * 10752 bytes at most
    if (width > MR_PNG_MAX_SIDE || height > MR_PNG_MAX_SIDE) return MR_ERR_NOTIMPL;
    PngParams p{};
    p.packed = packed;
    p.out = frames_out;
    p.frame_bytes = mr_png_packed_bytes(width, height, channels);
    p.H = height; p.W = width;
    p.stride = 1 + width * channels;
    p.groups = (width + 3) / 4;
    p.bands = (height + PNG_BAND - 1) / PNG_BAND;
    p.steps = p.groups + PNG_BAND - 1;
    p.last_dword = (int)(p.frame_bytes / 4) - 1;
    p.dword_stores = width % 4 == 0;
    const size_t lds = (size_t)p.groups * channels * 4;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)num_frames), block(MR_WAVE);
    switch (channels) {
        case 1: hipLaunchKernelGGL(png_unfilter_kernel<1>, grid, block, lds, s, p); break;
        case 2: hipLaunchKernelGGL(png_unfilter_kernel<2>, grid, block, lds, s, p); break;
        case 3: hipLaunchKernelGGL(png_unfilter_kernel<3>, grid, block, lds, s, p); break;
        default: hipLaunchKernelGGL(png_unfilter_kernel<4>, grid, block, lds, s, p); break;
    }
    MR_CHECK_LAUNCH();
    return MR_OK;
}
