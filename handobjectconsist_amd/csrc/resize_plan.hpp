// resize_plan.hpp -- the host side of mr_frames_resize (csrc/frame_resize.hip): Pillow's coefficient tables for a BILINEAR
// resize of 8-bit pixels, and what the launcher decides from the four sizes.  Plain C++17, no HIP include, no pointer into
// device memory and no runtime call: tests/test_resize_host.py reaches every function through the C-ABI on a CPU.
//
// The tables are Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) operation by operation, in
// IEEE double; the library is built with -ffp-contract=off, so no product and sum are fused.  Per axis, for output index i:
//   bounds[2 i] = lo, bounds[2 i + 1] = n: the taps are the source pixels lo .. lo + n - 1;
//   coeffs[i * taps + x], x < n: their 22-bit fixed-point weights; x >= n: 0 (the kernel's loops run over all `taps`).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/meshraster_hip.h"

namespace mr {

constexpr int RZ_TW = 32;             // output pixels a tile is wide: 96 bytes = 24 dwords of an intermediate row
constexpr int RZ_TH_MAX = 16;         // output rows a tile is high, at most (a power of two)
constexpr int RZ_THREADS = 256;
constexpr int RZ_PITCH = RZ_TW * 3;   // bytes of an intermediate row in LDS
constexpr int RZ_MAX_TAPS = 33;       // a reduction by 16
constexpr int RZ_PRECISION_BITS = 22; // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RZ_LDS_LIMIT = 64 * 1024;
// what a tile's intermediate rows may take before the plan halves the tile's height: several workgroups stay resident per
// compute unit (160 KB of LDS) at every factor
constexpr int RZ_ROWS_BUDGET = 16 * 1024;
// ... and what the strip of staged source rows may take: as many rows at a time as fit, RZ_CHUNK_MIN at least (two per wave;
// the widest strip, a reduction by 16, is 1664 bytes a row)
constexpr int RZ_STRIP_BUDGET = 16 * 1024;
constexpr int RZ_CHUNK_MIN = 8;
constexpr int RZ_STRIP_TAIL = 64;     // bytes behind the strip that the windowed horizontal pass may read (and never uses)

inline bool resize_side_ok(int size) { return size >= 1 && size <= MR_PNG_MAX_SIDE; }

// taps per output pixel of one axis (Pillow's ksize), or MR_ERR_BADARG / MR_ERR_NOTIMPL
inline int resize_taps(int in_size, int out_size) {
    if (in_size < 1 || out_size < 1) return MR_ERR_BADARG;
    if (!resize_side_ok(in_size) || !resize_side_ok(out_size)) return MR_ERR_NOTIMPL;
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;  // (the triangle filter's support is 1)
    const int taps = (int)std::ceil(support) * 2 + 1;
    return taps <= RZ_MAX_TAPS ? taps : MR_ERR_NOTIMPL;
}

inline double resize_bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

// The first source pixel and the count of the taps of output pixel i of one axis: the centre (i + 0.5) scale, the support
// max(scale, 1) either side, rounded as Pillow rounds and cut at the frame.
inline void resize_bounds_of(int in_size, int out_size, int i, int& lo, int& n) {
    const double scale = (double)in_size / out_size;
    const double support = 1.0 * (scale < 1.0 ? 1.0 : scale);
    const double center = (i + 0.5) * scale;
    lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in_size) hi = in_size;
    n = hi - lo;
}

// bounds[2 * out_size], coeffs[out_size * taps] of one axis; returns taps (or what resize_taps refuses with)
inline int resize_tables(int in_size, int out_size, int* bounds, int* coeffs) {
    const int taps = resize_taps(in_size, out_size);
    if (taps < 0) return taps;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    double w[RZ_MAX_TAPS];
    for (int i = 0; i < out_size; i++) {
        const double center = (i + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        int lo, n;
        resize_bounds_of(in_size, out_size, i, lo, n);
        double ww = 0.0;
        for (int x = 0; x < n; x++) {
            w[x] = resize_bilinear((x + lo - center + 0.5) * ss);
            ww += w[x];
        }
        int* k = coeffs + (int64_t)i * taps;
        for (int x = 0; x < taps; x++) {
            if (x >= n) {
                k[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << RZ_PRECISION_BITS)) : (int)(0.5 + v * (1 << RZ_PRECISION_BITS));
        }
        bounds[2 * i] = lo;
        bounds[2 * i + 1] = n;
    }
    return taps;
}

struct ResizePlan {
    int tile_w, tile_h;    // output pixels of a workgroup's tile
    int rows;              // intermediate rows a tile holds: the most source rows the taps of tile_h output rows span
    int lds_bytes;         // both axes' coefficients of the tile (ints), rows * RZ_PITCH bytes, chunk_rows * strip_pitch bytes, the tail
    int grid_x, grid_y;    // tiles across and down (grid z walks the frames)
    int cols;              // source columns a tile holds: the most the taps of tile_w output columns span
    int chunk_rows;        // source rows staged in LDS at a time (the strip), at most `rows`
    int strip_pitch;       // bytes of a staged source row: 3 * cols and up to 15 bytes in front of them, a multiple of 16
    int taps_x, taps_y;
};

// source pixels between the first tap of a tile's first output pixel and the last tap of its last along one axis, at most
// over the tiles of `tile` output pixels
inline int resize_span_held(int in_size, int out_size, int tile) {
    int span = 1;
    for (int t0 = 0; t0 < out_size; t0 += tile) {
        int first = in_size, last = 0;
        for (int i = t0; i < std::min(t0 + tile, out_size); i++) {
            int lo, n;
            resize_bounds_of(in_size, out_size, i, lo, n);
            first = std::min(first, lo);
            last = std::max(last, lo + n);
        }
        span = std::max(span, last - first);
    }
    return span;
}

// both axes' coefficients of a tile, up to the 16-byte alignment of what follows them in LDS
constexpr int resize_table_bytes(int tile_h, int taps_x, int taps_y) { return (4 * (RZ_TW * taps_x + tile_h * taps_y) + 15) & ~15; }

constexpr int resize_lds_bytes(int tile_h, int rows, int taps_x, int taps_y, int chunk_rows, int strip_pitch) {
    return resize_table_bytes(tile_h, taps_x, taps_y) + rows * RZ_PITCH + chunk_rows * strip_pitch + RZ_STRIP_TAIL;
}

// MR_OK, or what resize_taps refuses an axis with (the horizontal one first)
inline int resize_plan(int src_w, int src_h, int dst_w, int dst_h, ResizePlan& p) {
    const int tx = resize_taps(src_w, dst_w);
    if (tx < 0) return tx;
    const int ty = resize_taps(src_h, dst_h);
    if (ty < 0) return ty;
    p.taps_x = tx;
    p.taps_y = ty;
    p.tile_w = RZ_TW;
    p.tile_h = RZ_TH_MAX;
    p.rows = resize_span_held(src_h, dst_h, p.tile_h);
    while (p.tile_h > 1 && p.rows * RZ_PITCH > RZ_ROWS_BUDGET) {  // a lower tile for large factors
        p.tile_h /= 2;
        p.rows = resize_span_held(src_h, dst_h, p.tile_h);
    }
    p.cols = resize_span_held(src_w, dst_w, p.tile_w);
    p.strip_pitch = (3 * p.cols + 15 + 15) & ~15;
    p.chunk_rows = std::min(p.rows, std::max(RZ_CHUNK_MIN, RZ_STRIP_BUDGET / p.strip_pitch));
    p.lds_bytes = resize_lds_bytes(p.tile_h, p.rows, tx, ty, p.chunk_rows, p.strip_pitch);
    p.grid_x = (dst_w + p.tile_w - 1) / p.tile_w;
    p.grid_y = (dst_h + p.tile_h - 1) / p.tile_h;
    return p.lds_bytes <= RZ_LDS_LIMIT ? MR_OK : MR_ERR_NOTIMPL;
}

}  // namespace mr
