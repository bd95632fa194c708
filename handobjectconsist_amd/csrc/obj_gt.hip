// obj_gt.hip -- ground-truth object meshes from a device-resident model bank, for gfx950 (MI355X): what a DataLoader worker
// does per frame with get_obj_verts_trans / get_obj_verts_can / get_obj_faces and collate.pad_cyclic.
//
//   obj_bank_build_kernel  once per bank and device.  One workgroup of four waves per model: a segmented min / max over the
//       model's vertices (each thread its stride, the lanes of a wave by a butterfly, the four waves through LDS), the centre
//       (min + max) * 0.5f per axis -- libyana's center_vert_bbox(verts, scale=False) -- and the canonical copy v - centre,
//       stored one float per lane.  min, max, +, * 0.5f and - are one IEEE operation each and min / max are associative: the
//       result has numpy's float32 bits whatever the order.  Zeros of both signs are ordered -0 < +0 (np.min leaves that to
//       its SIMD width; datasets/objgt.py's host code orders them the same way).
//   obj_gt_batch_kernel    once per step, all frames of all collated dicts.  A workgroup owns 256 consecutive ROWS of the flat
//       vertex outputs (or of the face output, or 256 frames' centres and scales).  Phase 1, one lane per row: the row's frame
//       -- a bisection over the records' row offsets for the workgroup's FIRST row, which depends on the workgroup id alone
//       (scalar loads), then a walk forward from there, a step or two --, its slot in the frame, the source row (slot mod n)
//       of the frame's model with n from the bank's table (cyclic repetition, collate.pad_cyclic's rule), A v + b and all three
//       components of R y - c once, the canonical row; results to LDS at a stride of three dwords (no bank conflict).  Phase
//       2, one lane per OUTPUT element: 768 consecutive dwords of objverts3d and of objcanverts, or 768 consecutive qwords of
//       objfaces (int64: what the render path's C-ABI reads), stored densely.  The bank stays in L2: a step reads it many
//       times over.  No atomics, no workspace.  The OUTPUT index is formed from the workgroup and lane ids alone, below the
//       row counts the host was given and checked against the capacities; what comes from device memory only selects the
//       SOURCE, and every such value is clamped to its buffer first (model id to [0, M), a table row to the bank's extent;
//       a slot outside its frame's padded length is marked in LDS and written by nobody).
//
//   objverts3d = rot (A v + b) - c   one fp32 operation per operator, products summed left to right (-ffp-contract=off):
//       y_i = ((A_i0 v_0 + A_i1 v_1) + A_i2 v_2) + b_i,   out_r = ((R_r0 y_0 + R_r1 y_1) + R_r2 y_2) - c_r
//   rot carries the mirror (column 0 negated: exact), c is zero where HandObjSet centres nothing.
#include "mr_common.hpp"

#pragma clang fp contract(off)  // (the build's -ffp-contract=off, restated where bit-exactness is the contract)

namespace mr {

constexpr int OG_THREADS = 256, OG_WAVES = OG_THREADS / MR_WAVE;

// min / max in the total order of the bit patterns (-0 < +0); the inputs are finite
__device__ __forceinline__ float min_total(float a, float b) { return f2ord(b) < f2ord(a) ? b : a; }
__device__ __forceinline__ float max_total(float a, float b) { return f2ord(b) > f2ord(a) ? b : a; }

struct BankParams {
    const float* verts;    // [total_verts,3]
    const int32_t* table;  // [M,4]: first vertex, vertices, first face, faces
    float* box;            // [M,6]: min xyz, max xyz
    float* centre;         // [M,3]
    float* canverts;       // [total_verts,3]
    int total_verts;
};

// grid M
__global__ void __launch_bounds__(OG_THREADS) obj_bank_build_kernel(BankParams p) {
    __shared__ float red[OG_WAVES][6];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int start = p.table[4 * m], n = p.table[4 * m + 1];
    // (the table is device data: a row that leaves the bank is skipped by the whole workgroup)
    if (n < 1 || start < 0 || start > p.total_verts - n) return;
    const float* v = p.verts + (int64_t)start * 3;
    float lo[3], hi[3];
#pragma unroll
    for (int r = 0; r < 3; r++) lo[r] = hi[r] = v[r];  // (vertex 0: a thread without a vertex of its own changes nothing)
    for (int i = tid; i < n; i += OG_THREADS) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float x = v[3 * (int64_t)i + r];
            lo[r] = min_total(lo[r], x);
            hi[r] = max_total(hi[r], x);
        }
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo[r] = min_total(lo[r], __shfl_xor(lo[r], off));
            hi[r] = max_total(hi[r], __shfl_xor(hi[r], off));
        }
        if (lane == 0) { red[wave][r] = lo[r]; red[wave][3 + r] = hi[r]; }
    }
    __syncthreads();
    float c[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        lo[r] = red[0][r]; hi[r] = red[0][3 + r];
#pragma unroll
        for (int w = 1; w < OG_WAVES; w++) { lo[r] = min_total(lo[r], red[w][r]); hi[r] = max_total(hi[r], red[w][3 + r]); }
        c[r] = (lo[r] + hi[r]) * 0.5f;
    }
    if (tid < 3) {
        const float l = tid == 0 ? lo[0] : tid == 1 ? lo[1] : lo[2], h = tid == 0 ? hi[0] : tid == 1 ? hi[1] : hi[2];
        p.box[6 * m + tid] = l;
        p.box[6 * m + 3 + tid] = h;
        p.centre[3 * m + tid] = tid == 0 ? c[0] : tid == 1 ? c[1] : c[2];
    }
    // t and t + 256 k differ by k modulo 3 (256 = 3 * 85 + 1): the component walks with the loop
    float* can = p.canverts + (int64_t)start * 3;
    const int64_t n3 = 3 * (int64_t)n;
    for (int64_t t = tid; t < n3; t += OG_THREADS) { const int r = (int)(t % 3); can[t] = v[t] - (r == 0 ? c[0] : r == 1 ? c[1] : c[2]); }
}

struct GtParams {
    const float* verts;       // the bank
    const float* canverts;
    const float* centre;
    const int32_t* faces;
    const int32_t* table;
    const MrObjFrame* frames;  // [N]
    float* objverts3d;
    float* objcanverts;
    int64_t* objfaces;
    float* objcantrans;        // [N,3]
    float* objcanscale;        // [N]
    int vert_rows, face_rows;
    int vert_blocks, face_blocks;  // workgroups of OG_THREADS rows
    int num_models, total_verts, total_faces, num_frames;
};

// The frame that holds `row`: the last one whose first row is at or below it.  `first` is the workgroup's first row, the same
// in every lane: the bisection's loads are scalar.  Offsets ascend, as the host lays them out; any other content still ends in
// [0, N) after at most N steps.
template <bool FACES>
__device__ __forceinline__ int frame_of(const MrObjFrame* __restrict__ frames, int n, int first, int row) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((FACES ? frames[mid].face_offset : frames[mid].vert_offset) <= first) lo = mid; else hi = mid - 1;
    }
    while (lo + 1 < n && (FACES ? frames[lo + 1].face_offset : frames[lo + 1].vert_offset) <= row) lo++;
    return lo;
}

// rows [first, first + n) of a bank array of `total` rows, whatever the table holds
__device__ __forceinline__ void bank_rows(const int32_t* table, int model, int num_models, int which, int total, int& first, int& n) {
    const int m = min(max(model, 0), num_models - 1);
    n = min(max(table[4 * m + 2 * which + 1], 1), total);
    first = min(max(table[4 * m + 2 * which], 0), total - n);
}

// grid vert_blocks + face_blocks + ceil(4 N / 256)
__global__ void __launch_bounds__(OG_THREADS) obj_gt_batch_kernel(GtParams p) {
    __shared__ float sa[3 * OG_THREADS];  // objverts3d rows; the face rows as int bit patterns
    __shared__ float sb[3 * OG_THREADS];  // objcanverts rows
    __shared__ unsigned char written[OG_THREADS];
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    if (blk < p.vert_blocks) {
        const int first = blk * OG_THREADS, row = first + tid;
        bool ok = false;
        if (row < p.vert_rows) {
            const MrObjFrame* f = p.frames + frame_of<false>(p.frames, p.num_frames, first, row);
            const int slot = row - f->vert_offset;
            if (slot >= 0 && slot < f->padded_verts) {
                int start, n;
                bank_rows(p.table, f->model, p.num_models, 0, p.total_verts, start, n);
                const int64_t src = 3 * (int64_t)(start + slot % n);
                const float v0 = p.verts[src], v1 = p.verts[src + 1], v2 = p.verts[src + 2];
                const float* A = f->pose;
                const float y0 = ((A[0] * v0 + A[1] * v1) + A[2] * v2) + A[3];
                const float y1 = ((A[4] * v0 + A[5] * v1) + A[6] * v2) + A[7];
                const float y2 = ((A[8] * v0 + A[9] * v1) + A[10] * v2) + A[11];
                const float* R = f->rot;
#pragma unroll
                for (int r = 0; r < 3; r++) sa[3 * tid + r] = ((R[3 * r] * y0 + R[3 * r + 1] * y1) + R[3 * r + 2] * y2) - f->center3d[r];
                const float c0 = p.canverts[src];
                sb[3 * tid] = f->flip ? -c0 : c0;
                sb[3 * tid + 1] = p.canverts[src + 1];
                sb[3 * tid + 2] = p.canverts[src + 2];
                ok = true;
            }
        }
        written[tid] = ok;
        __syncthreads();
        // (lane t and t + 256 k: element 256 k + t of the workgroup's 768, row (256 k + t) / 3)
        const int items = 3 * min(OG_THREADS, p.vert_rows - first);
        const int64_t base = 3 * (int64_t)first;
        for (int e = tid; e < items; e += OG_THREADS) {
            if (!written[e / 3]) continue;
            p.objverts3d[base + e] = sa[e];
            p.objcanverts[base + e] = sb[e];
        }
        return;
    }
    blk -= p.vert_blocks;
    if (blk < p.face_blocks) {
        int* si = reinterpret_cast<int*>(sa);
        const int first = blk * OG_THREADS, row = first + tid;
        bool ok = false;
        if (row < p.face_rows) {
            const MrObjFrame* f = p.frames + frame_of<true>(p.frames, p.num_frames, first, row);
            const int slot = row - f->face_offset;
            if (slot >= 0 && slot < f->padded_faces) {
                int start, n;
                bank_rows(p.table, f->model, p.num_models, 1, p.total_faces, start, n);
                const int64_t src = 3 * (int64_t)(start + slot % n);
#pragma unroll
                for (int r = 0; r < 3; r++) si[3 * tid + r] = p.faces[src + r];
                ok = true;
            }
        }
        written[tid] = ok;
        __syncthreads();
        const int items = 3 * min(OG_THREADS, p.face_rows - first);
        const int64_t base = 3 * (int64_t)first;
        for (int e = tid; e < items; e += OG_THREADS)
            if (written[e / 3]) p.objfaces[base + e] = (int64_t)si[e];
        return;
    }
    blk -= p.face_blocks;
    const int64_t k = (int64_t)blk * OG_THREADS + tid;
    if (k < 4 * (int64_t)p.num_frames) {
        const int fr = (int)(k >> 2), r = (int)(k & 3);
        const int m = min(max(p.frames[fr].model, 0), p.num_models - 1);
        if (r < 3) p.objcantrans[3 * fr + r] = p.centre[3 * m + r];
        else p.objcanscale[fr] = 1.0f;  // center_vert_bbox(scale=False)
    }
}

}  // namespace mr

using namespace mr;

extern "C" int mr_obj_bank_build(const float* verts, const int32_t* table, int num_models, int total_verts, float* box,
                                 float* centre, float* canverts, mr_stream_t stream) {
    if (num_models < 0 || total_verts < 0) return MR_ERR_BADARG;
    if (num_models == 0) return MR_OK;
    if (total_verts < 1 || !verts || !table || !box || !centre || !canverts) return MR_ERR_BADARG;
    if (misaligned({verts, table, box, centre, canverts}, 3)) return MR_ERR_BADARG;
    BankParams p{};  // (value-initialised, then filled: padding bytes are kernel-argument bytes like any other)
    p.verts = verts; p.table = table; p.box = box; p.centre = centre; p.canverts = canverts; p.total_verts = total_verts;
    hipLaunchKernelGGL(obj_bank_build_kernel, dim3((unsigned)num_models), dim3(OG_THREADS), 0, (hipStream_t)stream, p);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_obj_gt_batch(const float* verts, const float* canverts, const float* centre, const int32_t* faces,
                               const int32_t* table, int num_models, int total_verts, int total_faces, const MrObjFrame* frames,
                               int num_frames, int64_t vert_rows, int64_t face_rows, float* objverts3d, float* objcanverts,
                               int64_t vert_capacity, int64_t* objfaces, int64_t face_capacity, float* objcantrans,
                               float* objcanscale, mr_stream_t stream) {
    if (num_frames < 0 || num_models < 0 || total_verts < 0 || total_faces < 0 || vert_rows < 0 || face_rows < 0 ||
        vert_capacity < 0 || face_capacity < 0)
        return MR_ERR_BADARG;
    if (vert_rows > vert_capacity || face_rows > face_capacity || vert_rows > 0x7fffffffLL - OG_THREADS || face_rows > 0x7fffffffLL - OG_THREADS)  // (a workgroup's last row id is an int)
        return MR_ERR_BADARG;
    if (num_frames == 0) return (vert_rows == 0 && face_rows == 0) ? MR_OK : MR_ERR_BADARG;
    if (num_models < 1 || total_verts < 1 || total_faces < 1) return MR_ERR_BADARG;
    if (!verts || !canverts || !centre || !faces || !table || !frames || !objcantrans || !objcanscale) return MR_ERR_BADARG;
    if ((vert_rows && (!objverts3d || !objcanverts)) || (face_rows && !objfaces)) return MR_ERR_BADARG;
    if (misaligned({verts, canverts, centre, faces, table, frames, objverts3d, objcanverts, objcantrans, objcanscale}, 3) ||
        misaligned({objfaces}, 7))
        return MR_ERR_BADARG;
    GtParams p{};
    p.verts = verts; p.canverts = canverts; p.centre = centre; p.faces = faces; p.table = table; p.frames = frames;
    p.objverts3d = objverts3d; p.objcanverts = objcanverts; p.objfaces = objfaces; p.objcantrans = objcantrans;
    p.objcanscale = objcanscale; p.vert_rows = (int)vert_rows; p.face_rows = (int)face_rows;
    p.vert_blocks = (int)blocks1d(vert_rows); p.face_blocks = (int)blocks1d(face_rows);
    p.num_models = num_models; p.total_verts = total_verts; p.total_faces = total_faces; p.num_frames = num_frames;
    // (one thread per row, per face row and per centre / scale value: blocks1d of each, laid end to end)
    const int64_t blocks = (int64_t)p.vert_blocks + p.face_blocks + blocks1d(4 * (int64_t)num_frames);
    return launch1d(obj_gt_batch_kernel, blocks * OG_THREADS, (hipStream_t)stream, p);
}
