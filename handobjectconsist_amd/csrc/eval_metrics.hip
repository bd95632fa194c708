// eval_metrics.hip -- the training metrics of meshreg/netscripts/evaluate.py and libyana's EvalUtil for gfx950 (MI355X):
// what the reference computes on the host behind six pipeline drains per fed frame, from device tensors and without a
// host read.
//
// mr_eval_feed: ONE launch for everything a frame feeds.  Up to MR_EVAL_MAX_JOBS jobs travel by value in the kernel's
// argument block; grid (sample, job), one workgroup of four waves each.  A job is "distances between pred[b] and
// target[b]", optionally with one side taken through inverse(affine[b]) (recover_back) and both sides re-centred on a
// keypoint, written per point into the evaluator's log or summed per sample for a meter (a third mode writes the pred
// side's points themselves: recover_back as a function).  The caller offsets `out` to the
// row this feed starts at: no cursor on the device, no atomics, nothing read back.
//
// mr_eval_measures: the read-out of one evaluator's [rows, K] log.  One workgroup of 1024 threads per keypoint.  Pass 0
// copies the keypoint's column into the workspace (contiguous from then on), sums it in fp64 (thread-strided partials, a
// butterfly over the lanes, the sixteen waves in order), counts the non-finite rows and bins every row by a binary search
// over the thresholds held in LDS into an integer LDS histogram, whose inclusive scan is the PCK count.  The two middle
// order statistics come from a radix select over the order-preserving bit patterns of the column: four passes of eight
// bits, each an integer LDS histogram of 256 bins, per statistic.  Integer LDS atomics are order-free and cheap on this
// part; nothing here uses a floating-point atomic, and nothing is sorted.
#include "mr_common.hpp"

namespace mr {

constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / MR_WAVE;
constexpr int EV_MAX_POINTS = 4096;     // per-point jobs: the widest row of an evaluator's log
constexpr int EM_THREADS = 1024, EM_WAVES = EM_THREADS / MR_WAVE;
constexpr int EM_MAX_THRESHOLDS = 1024;  // one thread per threshold in the scan

struct EvalFeedArgs {
    MrEvalJob job[MR_EVAL_MAX_JOBS];
};

// rows 0 and 1 of inverse(a): adjugate over the determinant of the full 3 x 3, one IEEE operation per operator
__device__ __forceinline__ void affine_inverse_rows(const float* __restrict__ a, float (&inv)[6]) {
    const float c00 = a[4] * a[8] - a[5] * a[7], c01 = a[2] * a[7] - a[1] * a[8], c02 = a[1] * a[5] - a[2] * a[4];
    const float c10 = a[5] * a[6] - a[3] * a[8], c11 = a[0] * a[8] - a[2] * a[6], c12 = a[2] * a[3] - a[0] * a[5];
    const float c20 = a[3] * a[7] - a[4] * a[6];
    const float det = (a[0] * c00 + a[1] * c10) + a[2] * c20;
    inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
    inv[3] = c10 / det; inv[4] = c11 / det; inv[5] = c12 / det;
}

// point k of a sample's [K,dims] points (a third component of 0 for dims 2), through rows 0, 1 of the inverse affine
// when `recover`
__device__ __forceinline__ void load_point(const float* __restrict__ pts, int k, int dims, bool recover, const float (&inv)[6],
                                           float (&v)[3]) {
    const float* q = pts + (int64_t)k * dims;
    v[0] = q[0]; v[1] = q[1]; v[2] = dims == 3 ? q[2] : 0.0f;
    if (recover) {
        const float x = v[0], y = v[1];
        v[0] = (inv[0] * x + inv[1] * y) + inv[2];
        v[1] = (inv[3] * x + inv[4] * y) + inv[5];
    }
}

__device__ __forceinline__ float eval_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// grid (B, jobs)
__global__ void __launch_bounds__(EV_THREADS) eval_feed_kernel(EvalFeedArgs args) {
    __shared__ float red[EV_WAVES];
    const MrEvalJob& job = args.job[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x, K = job.num_points, dims = job.dims;
    float inv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const bool has_affine = job.affine != nullptr;
    if (has_affine) affine_inverse_rows(job.affine + (int64_t)b * 9, inv);
    const bool rec_pred = has_affine && !job.affine_target, rec_target = has_affine && job.affine_target;
    const float* pred = job.pred + (int64_t)b * K * dims;
    const float* target = job.target + (int64_t)b * K * dims;  // (never read in MR_EVAL_POINTS, where it may be NULL)
    float cp[3] = {0.0f, 0.0f, 0.0f}, ct[3] = {0.0f, 0.0f, 0.0f};
    if (job.center >= 0) {
        load_point(pred, job.center, dims, rec_pred, inv, cp);
        if (job.mode != MR_EVAL_POINTS) load_point(target, job.center, dims, rec_target, inv, ct);
    }
    float acc = 0.0f;
    for (int k = tid; k < K; k += EV_THREADS) {
        float p[3], t[3];
        load_point(pred, k, dims, rec_pred, inv, p);
        if (job.mode == MR_EVAL_POINTS) {  // recover_back itself: the pred side as it enters the distance
            float* o = job.out + ((int64_t)b * K + k) * dims;
            o[0] = p[0] - cp[0]; o[1] = p[1] - cp[1];
            if (dims == 3) o[2] = p[2] - cp[2];
            continue;
        }
        load_point(target, k, dims, rec_target, inv, t);
        const float d0 = (p[0] - cp[0]) - (t[0] - ct[0]);
        const float d1 = (p[1] - cp[1]) - (t[1] - ct[1]);
        const float d2 = (p[2] - cp[2]) - (t[2] - ct[2]);
        const float dist = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        if (job.mode == MR_EVAL_PER_POINT) job.out[(int64_t)b * K + k] = dist;
        else acc += dist;
    }
    if (job.mode != MR_EVAL_PER_SAMPLE_SUM) return;  // (uniform over the workgroup)
    // thread-strided partials, the lanes by the butterfly, the four waves in order
    acc = eval_wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = red[0];
        for (int w = 1; w < EV_WAVES; w++) s += red[w];
        job.out[b] = s;
    }
}

// NaN of either sign -> the largest key (np.sort's place for it); everything else in its numeric order
__device__ __forceinline__ uint32_t select_key(float x) { return x != x ? 0xffffffffu : f2ord(x); }
__device__ __forceinline__ float select_value(uint32_t key) { return key == 0xffffffffu ? __builtin_nanf("") : ord2f(key); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// grid K (one workgroup per keypoint); col = work + k * rows
__global__ void __launch_bounds__(EM_THREADS) eval_measures_kernel(const float* __restrict__ log, int rows, int num_kp,
                                                                   const float* __restrict__ thresholds, int T,
                                                                   double* __restrict__ sums, unsigned* __restrict__ pck_counts,
                                                                   float* __restrict__ mid, unsigned* __restrict__ nonfinite,
                                                                   float* __restrict__ work) {
    __shared__ float thr[EM_MAX_THRESHOLDS];
    __shared__ unsigned hist[EM_MAX_THRESHOLDS];
    __shared__ unsigned digit[256];
    __shared__ double wsum[EM_WAVES];
    __shared__ unsigned s_nonfinite, s_prefix, s_rank;
    const int k = blockIdx.x, tid = threadIdx.x;
    float* col = work + (int64_t)k * rows;
    if (tid < T) { thr[tid] = thresholds[tid]; hist[tid] = 0u; }
    if (tid == 0) s_nonfinite = 0u;
    __syncthreads();
    // ---- pass 0: column copy, fp64 sum, non-finite count, threshold histogram
    double acc = 0.0;
    unsigned bad = 0u;
    for (int i = tid; i < rows; i += EM_THREADS) {
        const float d = log[(int64_t)i * num_kp + k];
        col[i] = d;
        acc += (double)d;
        if (!(fabsf(d) <= 3.4028234663852886e38f)) { bad++; continue; }
        // the first threshold with d <= thr[j] (thresholds are non-decreasing): d counts in bins j .. T - 1
        int lo = 0, hi = T;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (d <= thr[m]) hi = m; else lo = m + 1;
        }
        if (lo < T) atomicAdd(&hist[lo], 1u);
    }
    if (bad) atomicAdd(&s_nonfinite, bad);
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();  // (also: the column in `work` is visible to the whole workgroup from here on)
    if (tid == 0) {
        double s = wsum[0];
        for (int w = 1; w < EM_WAVES; w++) s += wsum[w];
        sums[k] = s;
        nonfinite[k] = s_nonfinite;
    }
    // ---- inclusive scan of the histogram: thread j owns bin j
    for (int off = 1; off < T; off <<= 1) {
        unsigned add = 0u;
        if (tid < T && tid >= off) add = hist[tid - off];
        __syncthreads();
        if (tid < T) hist[tid] += add;
        __syncthreads();
    }
    if (tid < T) pck_counts[(int64_t)k * T + tid] = hist[tid];
    // ---- the two middle order statistics (0-based ranks (rows - 1) / 2 and rows / 2)
    float lower = 0.0f;
    for (int s = 0; s < 2; s++) {
        unsigned prefix = 0u, rank = (unsigned)(s == 0 ? (rows - 1) / 2 : rows / 2);
        if (s == 1 && (rows & 1)) {  // an odd count: one middle element
            if (tid == 0) mid[2 * k + 1] = lower;
            break;
        }
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) digit[tid] = 0u;
            __syncthreads();
            const uint32_t high = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
            for (int i = tid; i < rows; i += EM_THREADS) {
                const uint32_t key = select_key(col[i]);
                if ((key & high) == prefix) atomicAdd(&digit[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {  // wave 0, all lanes: four bins a lane
                const unsigned c0 = digit[4 * tid], c1 = digit[4 * tid + 1], c2 = digit[4 * tid + 2], c3 = digit[4 * tid + 3];
                const unsigned mine = c0 + c1 + c2 + c3;
                const unsigned incl = (unsigned)wave_incl_sum((int)mine), excl = incl - mine;
                if (rank >= excl && rank < incl) {  // exactly one lane: the keys under `prefix` number more than `rank`
                    unsigned r = rank - excl, d = 0u;
                    if (r >= c0) { r -= c0; d = 1u;
                        if (r >= c1) { r -= c1; d = 2u;
                            if (r >= c2) { r -= c2; d = 3u; } } }
                    s_prefix = prefix | ((4u * tid + d) << shift);
                    s_rank = r;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            rank = s_rank;
        }
        lower = select_value(prefix);
        if (tid == 0) mid[2 * k + s] = lower;
    }
}

static int eval_job_check(const MrEvalJob& j) {
    if (j.mode != MR_EVAL_PER_POINT && j.mode != MR_EVAL_PER_SAMPLE_SUM && j.mode != MR_EVAL_POINTS) return MR_ERR_BADARG;
    if (!j.pred || !j.out || (!j.target && j.mode != MR_EVAL_POINTS)) return MR_ERR_BADARG;
    if (misaligned({j.pred, j.target, j.affine, j.out}, 3)) return MR_ERR_BADARG;
    if (j.dims != 2 && j.dims != 3) return MR_ERR_BADARG;
    if (j.num_points < 1 || j.center < -1 || j.center >= j.num_points) return MR_ERR_BADARG;
    if (j.affine && j.dims != 2) return MR_ERR_BADARG;
    if (j.mode == MR_EVAL_PER_POINT && j.num_points > EV_MAX_POINTS) return MR_ERR_BADARG;
    return MR_OK;
}

}  // namespace mr

using namespace mr;

extern "C" int mr_eval_job_layout(int* out, int n) {
    const int layout[] = {(int)sizeof(MrEvalJob),        (int)offsetof(MrEvalJob, pred),       (int)offsetof(MrEvalJob, target),
                          (int)offsetof(MrEvalJob, affine), (int)offsetof(MrEvalJob, out),        (int)offsetof(MrEvalJob, num_points),
                          (int)offsetof(MrEvalJob, dims),   (int)offsetof(MrEvalJob, center),     (int)offsetof(MrEvalJob, mode),
                          (int)offsetof(MrEvalJob, affine_target), (int)offsetof(MrEvalJob, reserved)};
    const int count = (int)(sizeof(layout) / sizeof(layout[0]));
    if (!out || n < 0) return MR_ERR_BADARG;
    for (int i = 0; i < count && i < n; i++) out[i] = layout[i];
    return count;
}

extern "C" int mr_eval_feed(const MrEvalJob* jobs, int num_jobs, int batch_size, mr_stream_t stream) {
    if (num_jobs < 0 || num_jobs > MR_EVAL_MAX_JOBS || batch_size < 0) return MR_ERR_BADARG;
    if (num_jobs == 0 || batch_size == 0) return MR_OK;
    if (!jobs) return MR_ERR_BADARG;
    EvalFeedArgs args{};  // (value-initialised: the unused jobs and the padding are kernel-argument bytes like any other)
    for (int i = 0; i < num_jobs; i++) {
        const int rc = eval_job_check(jobs[i]);
        if (rc != MR_OK) return rc;
        MrEvalJob& j = args.job[i];
        j.pred = jobs[i].pred; j.target = jobs[i].target; j.affine = jobs[i].affine; j.out = jobs[i].out;
        j.num_points = jobs[i].num_points; j.dims = jobs[i].dims; j.center = jobs[i].center; j.mode = jobs[i].mode;
        j.affine_target = jobs[i].affine_target != 0;
    }
    if (!grid_ok(batch_size)) return MR_ERR_BADARG;
    hipLaunchKernelGGL(eval_feed_kernel, dim3((unsigned)batch_size, (unsigned)num_jobs), dim3(EV_THREADS), 0, (hipStream_t)stream, args);
    MR_CHECK_LAUNCH();
    return MR_OK;
}

extern "C" int mr_eval_measures_workspace_floats(int rows, int num_kp, int num_thresholds) {
    if (rows < 0 || num_kp < 1 || num_thresholds < 0) return MR_ERR_BADARG;
    const int64_t floats = (int64_t)rows * num_kp;  // the log, one contiguous column per keypoint
    return floats <= 0x7fffffffLL ? (int)floats : MR_ERR_BADARG;
}

extern "C" int mr_eval_measures(const float* log, int rows, int num_kp, const float* thresholds, int num_thresholds, double* sums,
                                unsigned* pck_counts, float* mid, unsigned* nonfinite, float* work, mr_stream_t stream) {
    if (mr_eval_measures_workspace_floats(rows, num_kp, num_thresholds) < 0) return MR_ERR_BADARG;
    if (rows == 0) return MR_OK;
    if (!log || !sums || !mid || !nonfinite || !work || (num_thresholds > 0 && (!thresholds || !pck_counts))) return MR_ERR_BADARG;
    if (misaligned({log, thresholds, pck_counts, mid, nonfinite, work}, 3) || misaligned({sums}, 7)) return MR_ERR_BADARG;
    if (num_thresholds > EM_MAX_THRESHOLDS) return MR_ERR_NOTIMPL;
    hipLaunchKernelGGL(eval_measures_kernel, dim3((unsigned)num_kp), dim3(EM_THREADS), 0, (hipStream_t)stream, log, rows, num_kp,
                       thresholds, num_thresholds, sums, pck_counts, mid, nonfinite, work);
    MR_CHECK_LAUNCH();
    return MR_OK;
}
