// gt2d.hip -- 2-D ground truth from resident geometry, for gfx950 (MI355X): what a DataLoader worker does per frame with
// get_objverts2d / get_hand_verts2d / get_joints2d, HandObjSet's mirror (W - x), handutils.transform_coords and
// collate.pad_cyclic.
//
//   gt2d_batch_kernel    once per step: all frames of all collated dicts, all kinds of point.  The outputs are two flat
//       [rows,2] arrays -- the base pixels and the pixels after the crop affine -- and a RECORD (MrGt2dRecord) per (frame,
//       kind) says which rows are its own and where their points come from:
//         BANK      vertex (slot mod n) of a model of the resident bank, placed by p = A v + b -- obj_gt_batch_kernel's
//                   expression, parenthesis for parenthesis: p has the bits of the point that kernel rotates and centres;
//         POINTS3D  row (slot mod count) of the record's block of a dense [*,3] array of camera-frame points;
//         POINTS2D  row (slot mod count) of its block of a dense [*,2] array of base pixels: nothing is projected.
//       A workgroup owns 256 consecutive rows.  Phase 1, one lane per row: the row's record -- frame_of's bisection over the
//       records' first rows for the workgroup's FIRST row (it depends on the workgroup id alone: scalar loads), then a walk
//       forward --, the point, the three stages below; four floats to LDS, x and y in arrays of their own (a lane a bank).
//       Phase 2, one lane per OUTPUT element: 512 consecutive floats of each output, stored densely.  No atomics, no
//       workspace.  The OUTPUT index is formed from the workgroup and lane ids alone, below the row count the host was given
//       and checked against the capacity; what comes from device memory only selects the SOURCE, and every such value is
//       clamped to its buffer first (model id to [0, M), a table row to the bank's extent, a block of a dense array to the
//       array's rows); a slot outside its record's padded length is marked in LDS and written by nobody.
//
//   1. hom_r = (K_r0 p_0 + K_r1 p_1) + K_r2 p_2,  x = hom_0 / hom_2,  y = hom_1 / hom_2      fp32, one rounding per operator
//   2. x = W - x where the record is mirrored                                                 -> base
//   3. t_r = (double(M_r0) double(x) + double(M_r1) double(y)) + double(M_r2), rounded once   -> trans
//   hom_2 == 0 gives IEEE's inf / NaN in that row's elements, as numpy's division does.
#include "mr_common.hpp"  // (csrc/ is on the include path of a source in a subdirectory)

#pragma clang fp contract(off)  // (the build's -ffp-contract=off, restated where the order of roundings is the contract)

namespace mr {

constexpr int G2_THREADS = 256;

struct Gt2dParams {
    const float* verts;          // the bank (may be absent: num_models == 0)
    const int32_t* table;
    const float* points3d;       // [rows3d,3]
    const float* points2d;       // [rows2d,2]
    const MrGt2dRecord* records; // [N]
    float* base;                 // [rows,2]
    float* trans;                // [rows,2]
    int rows, num_records;
    int num_models, total_verts, rows3d, rows2d;
};

// The record that holds `row`: the last one whose first row is at or below it.  `first` is the workgroup's first row, the same
// in every lane: the bisection's loads are scalar.  Offsets ascend, as the host lays them out; any other content still ends in
// [0, N) after at most N steps.
__device__ __forceinline__ int record_of(const MrGt2dRecord* __restrict__ rec, int n, int first, int row) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rec[mid].row_offset <= first) lo = mid; else hi = mid - 1;
    }
    while (lo + 1 < n && rec[lo + 1].row_offset <= row) lo++;
    return lo;
}

// rows [first, first + n) of an array of `total` >= 1 rows, whatever the record says
__device__ __forceinline__ void dense_rows(int want_first, int want_n, int total, int& first, int& n) {
    n = min(max(want_n, 1), total);
    first = min(max(want_first, 0), total - n);
}

// grid ceil(rows / 256)
__global__ void __launch_bounds__(G2_THREADS) gt2d_batch_kernel(Gt2dParams p) {
    __shared__ float sbx[G2_THREADS], sby[G2_THREADS], stx[G2_THREADS], sty[G2_THREADS];
    __shared__ unsigned char written[G2_THREADS];
    const int tid = threadIdx.x;
    const int first = blockIdx.x * G2_THREADS, row = first + tid;
    bool ok = false;
    if (row < p.rows) {
        const MrGt2dRecord* f = p.records + record_of(p.records, p.num_records, first, row);
        const int slot = row - f->row_offset;
        if (slot >= 0 && slot < f->padded) {
            float x = 0.0f, y = 0.0f;
            bool have = true;
            if (f->mode == MR_GT2D_POINTS2D) {
                have = p.rows2d > 0;
                if (have) {
                    int start, n;
                    dense_rows(f->src_first, f->count, p.rows2d, start, n);
                    const int64_t src = 2 * (int64_t)(start + slot % n);
                    x = p.points2d[src];
                    y = p.points2d[src + 1];
                }
            } else {
                float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
                if (f->mode == MR_GT2D_BANK) {
                    have = p.num_models > 0;
                    if (have) {
                        const int m = min(max(f->model, 0), p.num_models - 1);
                        int start, n;
                        dense_rows(p.table[4 * m], p.table[4 * m + 1], p.total_verts, start, n);
                        const int64_t src = 3 * (int64_t)(start + slot % n);
                        const float v0 = p.verts[src], v1 = p.verts[src + 1], v2 = p.verts[src + 2];
                        const float* A = f->pose;
                        p0 = ((A[0] * v0 + A[1] * v1) + A[2] * v2) + A[3];
                        p1 = ((A[4] * v0 + A[5] * v1) + A[6] * v2) + A[7];
                        p2 = ((A[8] * v0 + A[9] * v1) + A[10] * v2) + A[11];
                    }
                } else {
                    have = p.rows3d > 0;
                    if (have) {
                        int start, n;
                        dense_rows(f->src_first, f->count, p.rows3d, start, n);
                        const int64_t src = 3 * (int64_t)(start + slot % n);
                        p0 = p.points3d[src]; p1 = p.points3d[src + 1]; p2 = p.points3d[src + 2];
                    }
                }
                const float* K = f->K;
                const float h0 = (K[0] * p0 + K[1] * p1) + K[2] * p2;
                const float h1 = (K[3] * p0 + K[4] * p1) + K[5] * p2;
                const float h2 = (K[6] * p0 + K[7] * p1) + K[8] * p2;
                x = h0 / h2;
                y = h1 / h2;
            }
            if (have) {  // (a record whose source array is absent -- the host refuses it -- leaves its rows unwritten)
                if (f->flip) x = f->width - x;
                const float* M = f->affine;
                sbx[tid] = x;
                sby[tid] = y;
                stx[tid] = (float)(((double)M[0] * (double)x + (double)M[1] * (double)y) + (double)M[2]);
                sty[tid] = (float)(((double)M[3] * (double)x + (double)M[4] * (double)y) + (double)M[5]);
                ok = true;
            }
        }
    }
    written[tid] = ok;
    __syncthreads();
    // (lane t and t + 256: element t and 256 + t of the workgroup's 512, row e / 2, component e & 1)
    const int items = 2 * min(G2_THREADS, p.rows - first);
    const int64_t out0 = 2 * (int64_t)first;
    for (int e = tid; e < items; e += G2_THREADS) {
        const int r = e >> 1;
        if (!written[r]) continue;
        p.base[out0 + e] = (e & 1) ? sby[r] : sbx[r];
        p.trans[out0 + e] = (e & 1) ? sty[r] : stx[r];
    }
}

}  // namespace mr

using namespace mr;

extern "C" int mr_gt2d_batch(const float* verts, const int32_t* table, int num_models, int total_verts, const float* points3d,
                             int64_t rows3d, const float* points2d, int64_t rows2d, const MrGt2dRecord* records, int num_records,
                             int64_t rows, float* base, float* trans, int64_t capacity, mr_stream_t stream) {
    if (num_records < 0 || num_models < 0 || total_verts < 0 || rows3d < 0 || rows2d < 0 || rows < 0 || capacity < 0) return MR_ERR_BADARG;
    if (rows > capacity || rows > 0x7fffffffLL - G2_THREADS || rows3d > 0x7fffffffLL || rows2d > 0x7fffffffLL)  // (a workgroup's last row id is an int)
        return MR_ERR_BADARG;
    if (num_records == 0) return rows == 0 ? MR_OK : MR_ERR_BADARG;
    if (rows == 0) return MR_OK;
    if (!records || !base || !trans) return MR_ERR_BADARG;
    if ((num_models > 0 && (total_verts < 1 || !verts || !table)) || (rows3d > 0 && !points3d) || (rows2d > 0 && !points2d)) return MR_ERR_BADARG;
    if (misaligned({verts, table, points3d, points2d, records, base, trans}, 3)) return MR_ERR_BADARG;
    Gt2dParams p{};  // (value-initialised, then filled: padding bytes are kernel-argument bytes like any other)
    p.verts = verts; p.table = table; p.points3d = points3d; p.points2d = points2d; p.records = records; p.base = base; p.trans = trans;
    p.rows = (int)rows; p.num_records = num_records; p.num_models = num_models; p.total_verts = total_verts;
    p.rows3d = (int)rows3d; p.rows2d = (int)rows2d;
    return launch1d(gt2d_batch_kernel, rows, (hipStream_t)stream, p);
}
