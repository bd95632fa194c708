// frame_resize.hip -- frames uint8 [N,Hs,Ws,3] -> uint8 [N,H,W,3] on gfx950, byte for byte what Pillow's
// Image.resize((W, H), Image.BILINEAR) gives (ImagingResample, src/libImaging/Resample.c): the triangle filter stretched by
// the reduction factor, two separable passes -- the horizontal one first -- over 22-bit fixed-point coefficients with an
// 8-bit intermediate image.  The tables come from the host (csrc/resize_plan.hpp), once per geometry.
//
//   frame_resize_kernel  A workgroup of 256 threads owns a tile of RZ_TW x tile_h output pixels of every frame grid z gives it.
//       Once: the tile's coefficients of both axes go to LDS (they are contiguous in the tables).  Per frame:
//       1. the source rows the tile's taps span are STAGED in LDS, chunk_rows at a time (the strip): 32 lanes take a row and
//          read the bytes the tile's columns span as aligned 16 bytes a lane, four rows' loads in flight per thread -- every
//          source byte is fetched once per tile, where per-tap loads of global memory fetched each cache line 27 times
//          (DESIGN 21 has the figures); a row starts wherever its address falls in its first 16 bytes (strip_pitch leaves
//          15 bytes for that);
//       2. barrier; horizontal pass: thread (row j, column x) sums the taps of output column x along staged row j and writes
//          the three rounded, clipped bytes to the intermediate row j in LDS (RZ_PITCH = 96 bytes a row: the tile's RGB
//          bytes, channel-agnostic from here on); barrier, next chunk.  Tap counts of 3, 5, 7 and 9 have an instantiation
//          that reads a column's window as dwords (rz_window_taps), any other count goes byte by byte;
//       3. vertical pass: a thread owns one DWORD of an output row of the tile -- four byte columns -- and sums the taps of
//          that output row down the intermediate rows, one LDS dword per tap;
//       4. it stores the dword where the output rows are dword-aligned (W a multiple of 4), its bytes elsewhere.
//       Every loop bound (rows, chunks, taps, tile height, frames) is a number the host computed from the sizes.  Every index
//       formed from a table entry is clamped to the frame, to the strip or to the rows held, and the taps past an entry's
//       count have weight 0, so tables of another geometry give wrong pixels and no access outside the buffers.  A chunk
//       of the strip that would end behind the last byte of frames_in (or any chunk of a frames_in that is not 16-byte
//       aligned) is put together from byte loads clamped to the tensor.
//
// One launch per call whatever N; no workspace, no scratch, no atomics, no float instruction (the one division is by the
// constant 24, a multiplication).
#include "mr_common.hpp"
#include "resize_plan.hpp"

namespace mr {

constexpr int RZ_ROW_DWORDS = RZ_PITCH / 4;
constexpr int RZ_STAGE_ROWS = 4;  // source rows a thread has in flight while staging (16 bytes each)
static_assert(RZ_TW == 32 && RZ_THREADS == 256, "the horizontal pass splits a thread index into 5 bits of column and 3 of row");
static_assert(RZ_PITCH % 4 == 0, "the vertical pass reads an intermediate row as dwords");
static_assert(RZ_MAX_TAPS == MR_RESIZE_MAX_TAPS, "the header states the cap");

struct ResizeParams {
    const uint8_t* in;   // [N,Hs,Ws,3]
    uint8_t* out;        // [N,H,W,3]
    const int* bounds_x; // [W][2]
    const int* coeffs_x; // [W][taps_x]
    const int* bounds_y; // [H][2]
    const int* coeffs_y; // [H][taps_y]
    int64_t in_frame, out_frame;  // bytes of a frame
    int64_t in_bytes;    // bytes of frames_in
    int N, Ws, Hs, W, H;
    int taps_x, taps_y;
    int tile_h;          // output rows of a tile
    int rows;            // intermediate rows a tile holds
    int cols;            // source columns a tile holds
    int chunk_rows;      // source rows staged at a time
    int strip_pitch;     // bytes of a staged row
    int in_aligned;      // frames_in is 16-byte aligned: the strip is loaded 16 bytes a lane
    int dword_stores;    // W % 4 == 0: every output row starts on a dword
};

__device__ __forceinline__ int rz_clip8(unsigned acc) {
    const int v = (int)acc >> RZ_PRECISION_BITS;  // (arithmetic shift, as Pillow's clip8)
    return min(max(v, 0), 255);
}

// 16 bytes of frames_in from byte offset `o` on, byte by byte with every index clamped to the tensor: the chunks that end
// behind frames_in's last byte (the last rows of the last frame), and every chunk of a tensor that is not 16-byte aligned
__device__ __forceinline__ unsigned rz_load4_bytes(const uint8_t* in, int64_t o, int64_t last) {
    return (unsigned)in[min(o, last)] | ((unsigned)in[min(o + 1, last)] << 8) | ((unsigned)in[min(o + 2, last)] << 16) |
           ((unsigned)in[min(o + 3, last)] << 24);
}
__device__ __forceinline__ uint4 rz_load16_bytes(const uint8_t* in, int64_t o, int64_t in_bytes) {
    const int64_t last = in_bytes - 1;
    return make_uint4(rz_load4_bytes(in, o, last), rz_load4_bytes(in, o + 4, last), rz_load4_bytes(in, o + 8, last),
                      rz_load4_bytes(in, o + 12, last));
}

// The horizontal taps of one output pixel where their count is a compile-time number: the 3 TAPS bytes from byte `byte0`
// of a staged row on, read as the dwords that hold them (one more than they fill: they begin anywhere in the first),
// realigned by v_alignbyte, each byte then at a fixed place.  Where a pixel has fewer taps (the frame's edges) the bytes behind
// them have weight 0, whatever they are; behind the strip's last row they are RZ_STRIP_TAIL bytes nobody wrote.
template <int TAPS>
__device__ __forceinline__ void rz_window_taps(const uint8_t* row, int byte0, const unsigned (&k)[TAPS], unsigned& a0, unsigned& a1, unsigned& a2) {
    constexpr int NQ = (3 * TAPS + 3) / 4;
    static_assert(4 * (NQ + 1) <= RZ_STRIP_TAIL, "the window of a row's last column ends inside the strip's tail");
    const unsigned* wp = reinterpret_cast<const unsigned*>(row) + (byte0 >> 2);
    unsigned w[NQ + 1], q[NQ];
#pragma unroll
    for (int i = 0; i <= NQ; i++) w[i] = wp[i];
#pragma unroll
    for (int i = 0; i < NQ; i++) q[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], (unsigned)byte0 & 3u);
#pragma unroll
    for (int t = 0; t < TAPS; t++) {
        a0 += ((q[(3 * t) >> 2] >> (8 * ((3 * t) & 3))) & 255u) * k[t];
        a1 += ((q[(3 * t + 1) >> 2] >> (8 * ((3 * t + 1) & 3))) & 255u) * k[t];
        a2 += ((q[(3 * t + 2) >> 2] >> (8 * ((3 * t + 2) & 3))) & 255u) * k[t];
    }
}

// TAPS_X: the horizontal taps where the launcher has an instantiation for their count (3: enlargements and the identity,
// 5, 7, 9: reductions up to 2, 3, 4), 0: any count, byte by byte
template <int TAPS_X>
__global__ __launch_bounds__(RZ_THREADS) void frame_resize_kernel(ResizeParams p) {
    extern __shared__ int rz_lds[];
    int* kx = rz_lds;                       // [RZ_TW][taps_x]
    int* ky = kx + RZ_TW * p.taps_x;        // [tile_h][taps_y]
    uint8_t* inter = reinterpret_cast<uint8_t*>(rz_lds) + resize_table_bytes(p.tile_h, p.taps_x, p.taps_y);  // [rows][RZ_PITCH]
    uint8_t* strip = inter + p.rows * RZ_PITCH;  // [chunk_rows][strip_pitch], 16-byte aligned
    const unsigned* inter_w = reinterpret_cast<const unsigned*>(inter);
    uint4* strip_v = reinterpret_cast<uint4*>(strip);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * RZ_TW, y0 = blockIdx.y * p.tile_h;
    const int vw = min(RZ_TW, p.W - x0), vh = min(p.tile_h, p.H - y0);  // the tile's valid pixels (both >= 1)

    for (int i = tid; i < vw * p.taps_x; i += RZ_THREADS) kx[i] = p.coeffs_x[x0 * p.taps_x + i];
    for (int i = tid; i < vh * p.taps_y; i += RZ_THREADS) ky[i] = p.coeffs_y[y0 * p.taps_y + i];
    const int row_first = min(max(p.bounds_y[2 * y0], 0), p.Hs - 1);
    const int col_first = min(max(p.bounds_x[2 * x0], 0), p.Ws - 1);
    const int xt = tid & (RZ_TW - 1);       // this thread's column of the horizontal pass
    const int xl = min(xt, vw - 1);         // (columns past the frame repeat the last one: their bytes are never stored)
    const int lo_rel = min(max(p.bounds_x[2 * (x0 + xl)], 0), p.Ws - 1) - col_first;
    const int hi_rel = min(p.cols, p.Ws - col_first) - 1;  // the last staged column that is a column of the frame (>= 0)
    const int* kxl = kx + xl * p.taps_x;
    const int valid_bytes = vw * 3;
    const int pitch_units = p.strip_pitch / 16;
    __syncthreads();
    unsigned kreg[TAPS_X > 0 ? TAPS_X : 1];  // this thread's column's weights (the windowed path)
#pragma unroll
    for (int k = 0; k < TAPS_X; k++) kreg[k] = (unsigned)kxl[k];
    const int lo_byte = min(max(lo_rel, 0), hi_rel) * 3;

    for (int n = blockIdx.z; n < p.N; n += gridDim.z) {
        const int64_t tile_off = (int64_t)n * p.in_frame + col_first * 3;  // + row * Ws * 3: a staged row's first byte
        for (int c0 = 0; c0 < p.rows; c0 += p.chunk_rows) {
            const int nc = min(p.chunk_rows, p.rows - c0);
            // 32 lanes a row, 16 bytes a lane.  A staged row ends within strip_pitch bytes of its first byte; where that is
            // inside the tensor for the chunk's last row (uniform over the workgroup), every load is one aligned 16 bytes
            // and RZ_STAGE_ROWS rows' loads are in flight per thread before the first LDS store
            const int64_t chunk_end = tile_off + (int64_t)min(row_first + c0 + nc - 1, p.Hs - 1) * (p.Ws * 3) + p.strip_pitch;
            if (p.in_aligned && chunk_end <= p.in_bytes) {
                for (int cb = tid >> 5; cb < nc; cb += RZ_STAGE_ROWS * (RZ_THREADS / 32)) {
                    for (int u = tid & 31; u < pitch_units; u += 32) {
                        uint4 v[RZ_STAGE_ROWS];
#pragma unroll
                        for (int i = 0; i < RZ_STAGE_ROWS; i++) {
                            // (rows past the chunk repeat its last one: a load more, no branch around it, nothing stored)
                            const int c = min(cb + i * (RZ_THREADS / 32), nc - 1);
                            const int64_t start = tile_off + (int64_t)min(row_first + c0 + c, p.Hs - 1) * (p.Ws * 3);
                            v[i] = *reinterpret_cast<const uint4*>(p.in + (start & ~(int64_t)15) + 16 * u);
                        }
#pragma unroll
                        for (int i = 0; i < RZ_STAGE_ROWS; i++) {
                            const int c = cb + i * (RZ_THREADS / 32);
                            if (c < nc) strip_v[c * pitch_units + u] = v[i];
                        }
                    }
                }
            } else {
                for (int c = tid >> 5; c < nc; c += RZ_THREADS / 32) {
                    const int64_t start = tile_off + (int64_t)min(row_first + c0 + c, p.Hs - 1) * (p.Ws * 3);
                    for (int u = tid & 31; u < pitch_units; u += 32)
                        strip_v[c * pitch_units + u] = rz_load16_bytes(p.in, (start & ~(int64_t)15) + 16 * u, p.in_bytes);
                }
            }
            __syncthreads();
            for (int c = tid >> 5; c < nc; c += RZ_THREADS / RZ_TW) {
                const int j = c0 + c;
                const int sh = (int)((tile_off + (int64_t)min(row_first + j, p.Hs - 1) * (p.Ws * 3)) & 15);
                const uint8_t* row = strip + c * p.strip_pitch + sh;
                unsigned a0 = 1u << (RZ_PRECISION_BITS - 1), a1 = a0, a2 = a0;
                if constexpr (TAPS_X > 0) {
                    rz_window_taps<TAPS_X>(strip + c * p.strip_pitch, sh + lo_byte, kreg, a0, a1, a2);
                } else {
                    for (int k = 0; k < p.taps_x; k++) {
                        const uint8_t* px = row + min(max(lo_rel + k, 0), hi_rel) * 3;
                        const unsigned w = (unsigned)kxl[k];
                        a0 += px[0] * w;
                        a1 += px[1] * w;
                        a2 += px[2] * w;
                    }
                }
                uint8_t* dst = inter + j * RZ_PITCH + xt * 3;
                dst[0] = (uint8_t)rz_clip8(a0);
                dst[1] = (uint8_t)rz_clip8(a1);
                dst[2] = (uint8_t)rz_clip8(a2);
            }
            __syncthreads();  // the next chunk overwrites the strip; after the last one, the intermediate rows are complete
        }
        uint8_t* out_tile = p.out + (int64_t)n * p.out_frame + ((int64_t)y0 * p.W + x0) * 3;
        for (int it = tid; it < p.tile_h * RZ_ROW_DWORDS; it += RZ_THREADS) {
            const int y = it / RZ_ROW_DWORDS, d = it - y * RZ_ROW_DWORDS;
            if (y >= vh || 4 * d >= valid_bytes) continue;
            const int off = min(max(p.bounds_y[2 * (y0 + y)] - row_first, 0), p.rows - 1);
            const int* kyl = ky + y * p.taps_y;
            unsigned a0 = 1u << (RZ_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int k = 0; k < p.taps_y; k++) {
                const unsigned w = inter_w[min(off + k, p.rows - 1) * RZ_ROW_DWORDS + d];
                const unsigned c = (unsigned)kyl[k];
                a0 += (w & 255u) * c;
                a1 += ((w >> 8) & 255u) * c;
                a2 += ((w >> 16) & 255u) * c;
                a3 += (w >> 24) * c;
            }
            const unsigned b0 = (unsigned)rz_clip8(a0), b1 = (unsigned)rz_clip8(a1), b2 = (unsigned)rz_clip8(a2), b3 = (unsigned)rz_clip8(a3);
            uint8_t* dst = out_tile + (int64_t)y * p.W * 3 + 4 * d;
            if (p.dword_stores) {  // (then valid_bytes is a multiple of 12: the dword is whole)
                *reinterpret_cast<uint32_t*>(dst) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            } else {
                const int count = valid_bytes - 4 * d;  // >= 1
                dst[0] = (uint8_t)b0;
                if (count > 1) dst[1] = (uint8_t)b1;
                if (count > 2) dst[2] = (uint8_t)b2;
                if (count > 3) dst[3] = (uint8_t)b3;
            }
        }
        // (no barrier here: the next frame writes the strip, which the vertical pass does not read, and the intermediate
        // rows only behind the barrier that follows its first staging, which every wave reaches after its vertical pass)
    }
}

}  // namespace mr

extern "C" int mr_frames_resize_taps(int in_size, int out_size) { return mr::resize_taps(in_size, out_size); }

extern "C" int mr_frames_resize_tables(int in_size, int out_size, int* bounds, int* coeffs) {
    if (in_size < 1 || out_size < 1 || !bounds || !coeffs) return MR_ERR_BADARG;
    return mr::resize_tables(in_size, out_size, bounds, coeffs);
}

extern "C" int mr_frames_resize_plan(int src_w, int src_h, int dst_w, int dst_h, int* plan) {
    if (src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1 || !plan) return MR_ERR_BADARG;
    mr::ResizePlan p{};
    const int rc = mr::resize_plan(src_w, src_h, dst_w, dst_h, p);
    if (rc != MR_OK) return rc;
    const int fields[MR_RESIZE_PLAN_INTS] = {p.tile_w, p.tile_h, p.rows, p.lds_bytes, p.grid_x, p.grid_y, p.cols, p.chunk_rows};
    for (int i = 0; i < MR_RESIZE_PLAN_INTS; i++) plan[i] = fields[i];
    return MR_OK;
}

extern "C" int mr_frames_resize_workspace_bytes(int num_frames, int src_w, int src_h, int dst_w, int dst_h) {
    if (num_frames < 0 || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return MR_ERR_BADARG;
    mr::ResizePlan p{};
    const int rc = mr::resize_plan(src_w, src_h, dst_w, dst_h, p);
    return rc != MR_OK ? rc : 0;
}

extern "C" int mr_frames_resize(const unsigned char* frames_in, int num_frames, int src_w, int src_h,
                                unsigned char* frames_out, int dst_w, int dst_h, const int* bounds_x, const int* coeffs_x,
                                const int* bounds_y, const int* coeffs_y, void* workspace, mr_stream_t stream) {
    using namespace mr;
    (void)workspace;  // (none is needed: mr_frames_resize_workspace_bytes is 0)
    if (num_frames < 0 || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return MR_ERR_BADARG;
    if (num_frames == 0) return MR_OK;
    if (!frames_in || !frames_out || !bounds_x || !coeffs_x || !bounds_y || !coeffs_y) return MR_ERR_BADARG;
    if (misaligned({frames_out, bounds_x, coeffs_x, bounds_y, coeffs_y}, 3)) return MR_ERR_BADARG;
    ResizePlan plan{};
    const int rc = resize_plan(src_w, src_h, dst_w, dst_h, plan);
    if (rc != MR_OK) return rc;
    ResizeParams p{};
    p.in = frames_in;
    p.out = frames_out;
    p.bounds_x = bounds_x; p.coeffs_x = coeffs_x;
    p.bounds_y = bounds_y; p.coeffs_y = coeffs_y;
    p.in_frame = (int64_t)src_h * src_w * 3;   // (at most 10752^2 * 3 < 2^31: offsets inside a frame are 32-bit)
    p.out_frame = (int64_t)dst_h * dst_w * 3;
    p.in_bytes = p.in_frame * num_frames;
    p.N = num_frames; p.Ws = src_w; p.Hs = src_h; p.W = dst_w; p.H = dst_h;
    p.taps_x = plan.taps_x; p.taps_y = plan.taps_y;
    p.tile_h = plan.tile_h;
    p.rows = plan.rows;
    p.cols = plan.cols;
    p.chunk_rows = plan.chunk_rows;
    p.strip_pitch = plan.strip_pitch;
    p.in_aligned = !misaligned({frames_in}, 15);
    p.dword_stores = dst_w % 4 == 0;
    const dim3 grid((unsigned)plan.grid_x, (unsigned)plan.grid_y, (unsigned)std::min(num_frames, 65535)), block(RZ_THREADS);
    const size_t lds = (size_t)plan.lds_bytes;
    const hipStream_t s = (hipStream_t)stream;
    switch (plan.taps_x) {
        case 3: hipLaunchKernelGGL(frame_resize_kernel<3>, grid, block, lds, s, p); break;
        case 5: hipLaunchKernelGGL(frame_resize_kernel<5>, grid, block, lds, s, p); break;
        case 7: hipLaunchKernelGGL(frame_resize_kernel<7>, grid, block, lds, s, p); break;
        case 9: hipLaunchKernelGGL(frame_resize_kernel<9>, grid, block, lds, s, p); break;
        default: hipLaunchKernelGGL(frame_resize_kernel<0>, grid, block, lds, s, p); break;
    }
    MR_CHECK_LAUNCH();
    return MR_OK;
}
