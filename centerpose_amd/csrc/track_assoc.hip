// Track association on the device (track.DeepSortTracker): the appearance gallery of a DeepSort tracker and its cost matrix.
//   cp_track_cost_f32    : cost[s, t, d] = min over the ring rows g < glen[s, t] of the cosine distance between gallery row g of track
//                          slot (s, t) and the feature in detection slot d of stream s -- NearestNeighborDistanceMetric.distance with
//                          _nn_cosine_distance (demo/tracking/sort/nn_matching.py:78-96, :156-177) for every track of every stream in
//                          one launch -- and det[s, d] = (x1, y1, x2, y2, score) of the row in that slot, in the same buffer
//   cp_track_append_f32  : features copied into ring rows bit for bit, 1 / |row| beside them
//   cp_track_*_host, cp_linear_assignment_host : the sequential HOST twins and the assignment of track_host.h
//
// The cost kernel is a GEMM with a min-reduction on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32): ring rows are M, detection
// slots are N in tiles of 32 columns, K = 512.  One block = one (stream, track slot) and one column tile; wave w owns ring rows
// 32w .. 32w + 31.  A lane (row or column i = lane % 32, k-group g = lane / 32) loads float4s of 4 consecutive k straight from global
// memory -- k0 + 8j + 4g, j = 0..3: each 32-float chunk of a row is read whole by its two lanes -- and feeds them to 4 successive
// MFMAs, the k permutation A and B share (igemm.h).  Rows >= glen are never loaded (their A fragments are zero and they stay out of the
// min), a wave whose slice lies wholly beyond glen skips the product, blocks of skipped slots (glen = 0) write their +inf row and leave.
// 1 / |feature| comes from the B fragments the wave holds anyway; the min runs over the 16 accumulator rows of a lane, the lane pair
// (shfl 32), then across the waves through LDS.
//
// Judged against: the kernel reads every valid ring row once per column tile and nothing else of size, so its floor is
// (sum of glen) * 2 KB * ceil(q / 32) at the HBM rate (5 TB/s nominal: 64 tracks x 100 rows = 12.8 MB -> 2.6 us).  Measured once
// (rocprofv3 kernel trace under tools/track_ab.py, N = 4, 32 tracks with full rings of 100, q = 8; profiles/track_kernel_stats.txt):
// 30.2 us median against a floor of 1.3 us for those 6.55 MB -- 23x above it.  The kernel is latency-bound, not bandwidth-bound: one
// wave per 32 rows walks K in 16 dependent rounds of loads with nothing else resident on its CU to hide them.  Staging through LDS or
// splitting K across more waves is the open step; at 30 us per call it is 2 % of what track= adds to a run_batch call.
#include "common.h"
#include "igemm.h"
#include "track_host.h"

#define TA_THREADS 256
#define TA_COLS 32

__global__ __launch_bounds__(TA_THREADS) void track_cost_kernel(const float* __restrict__ gallery, const float* __restrict__ ginv,
                                                                 const int* __restrict__ glen, const float* __restrict__ features,
                                                                 const int* __restrict__ slots, const float* __restrict__ rows, int M, int S,
                                                                 int Tcap, int budget, int q, float* __restrict__ cost, float* __restrict__ det)
{
    __shared__ float smin[TA_THREADS / CP_WAVE][TA_COLS];
    const float inf = __builtin_inff();
    const int slot = blockIdx.x, s = slot / Tcap, t = slot - s * Tcap;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, g = lane >> 5;
    const int d = blockIdx.y * TA_COLS + col;
    const bool dcol = d < q;
    const int v = dcol ? slots[(size_t)s * q + d] : -1;
    const bool used = v >= 0 && v < S * M;
    if (t == 0 && tid < TA_COLS && dcol) {                  // the stream's first track slot also writes the stream's det rows
        float* o = det + ((size_t)s * q + d) * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) o[k] = used ? rows[(size_t)v * 56 + k] : 0.f;
    }
    int n = glen[slot];
    n = n > budget ? budget : n;
    if (n <= 0) {                                           // uniform over the block
        if (tid < TA_COLS && dcol) cost[(size_t)slot * q + d] = inf;
        return;
    }
    if (wave * 32 < n) {                                    // uniform over the wave
        const int row = wave * 32 + col;
        const bool arow = row < n;
        const float* ap = gallery + ((size_t)slot * budget + (arow ? row : 0)) * TH_DIM + g * 4;
        const float* bp = features + ((size_t)s * q + (dcol ? d : 0)) * TH_DIM + g * 4;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float ss = 0.f;
#pragma unroll 2
        for (int k0 = 0; k0 < TH_DIM; k0 += 32) {
            float4 a[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = arow ? ig_ldg4(ap + k0 + 8 * j) : zero;
                b[j] = dcol ? ig_ldg4(bp + k0 + 8 * j) : zero;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = ig_mfma<32>(a[j].x, b[j].x, acc);
                acc = ig_mfma<32>(a[j].y, b[j].y, acc);
                acc = ig_mfma<32>(a[j].z, b[j].z, acc);
                acc = ig_mfma<32>(a[j].w, b[j].w, acc);
                ss += b[j].x * b[j].x + b[j].y * b[j].y + b[j].z * b[j].z + b[j].w * b[j].w;
            }
        }
        ss += __shfl_xor(ss, 32);                           // the two k-groups of a column
        const float finv = 1.0f / sqrtf(ss);
        const float* gi = ginv + (size_t)slot * budget;
        float best = inf;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = wave * 32 + ig_row<32>(r, lane);
            if (rr < n) best = fminf(best, 1.f - acc[r] * gi[rr] * finv);
        }
        best = fminf(best, __shfl_xor(best, 32));
        if (lane < TA_COLS) smin[wave][lane] = best;
    }
    __syncthreads();
    if (tid < TA_COLS && dcol) {
        const int nw = (n + 31) >> 5;
        float best = smin[0][tid];
        for (int w = 1; w < nw; ++w) best = fminf(best, smin[w][tid]);
        cost[(size_t)slot * q + d] = used ? best : inf;
    }
}

// one block per table entry, one float4 per thread; the sum of squares in the fixed order of th_tree_sumsq
__global__ __launch_bounds__(TH_LANES) void track_append_kernel(float* __restrict__ gallery, float* __restrict__ ginv,
                                                                const float* __restrict__ features, const int* __restrict__ table, int budget)
{
    __shared__ double p[TH_LANES];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int fs = table[3 * (size_t)i], ts = table[3 * (size_t)i + 1], pos = table[3 * (size_t)i + 2];
    if (fs < 0 || ts < 0 || pos < 0 || pos >= budget) return;       // uniform over the block
    const size_t row = (size_t)ts * budget + pos;
    const float4 x = ig_ldg4(features + (size_t)fs * TH_DIM + 4 * tid);
    *reinterpret_cast<float4*>(gallery + row * TH_DIM + 4 * tid) = x;
    p[tid] = th_lane_sumsq(x.x, x.y, x.z, x.w);
    __syncthreads();
    for (int s = TH_LANES / 2; s >= 1; s >>= 1) {
        if (tid < s) p[tid] += p[tid + s];
        __syncthreads();
    }
    if (tid == 0) ginv[row] = th_inv_norm(p[0]);
}

// per-row track ids, two launches so that nothing is ordered between workgroups inside one: every row gets -1, then every used and
// matched detection slot writes its id into its row.  Slots address distinct rows; a slot outside [0, S * M) is skipped.
__global__ __launch_bounds__(TA_THREADS) void track_row_ids_fill_kernel(int* __restrict__ row_ids, int total)
{
    const int r = blockIdx.x * TA_THREADS + threadIdx.x;
    if (r < total) row_ids[r] = -1;
}

__global__ __launch_bounds__(TA_THREADS) void track_row_ids_scatter_kernel(const int* __restrict__ slots, const int* __restrict__ slot_ids,
                                                                            int n, int total, int* __restrict__ row_ids)
{
    const int i = blockIdx.x * TA_THREADS + threadIdx.x;
    if (i >= n) return;
    const int v = slots[i], id = slot_ids[i];
    if (v >= 0 && v < total && id >= 0) row_ids[v] = id;
}

#define TA_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

static bool ta_aligned16(const void* p) { return (((size_t)p) & 15) == 0; }

extern "C" int cp_track_cost_host(const float* gallery, const float* ginv, const int* glen, const float* features, const int* slots,
                                  const float* rows, int M, int S, int Tcap, int budget, int q, float* out)
{
    TA_FORWARD(th_cost_host(gallery, ginv, glen, features, slots, rows, M, S, Tcap, budget, q, out, err, errn));
    return 0;
}

extern "C" int cp_track_append_host(float* gallery, float* ginv, const float* features, const int* table, int n, int budget)
{
    TA_FORWARD(th_append_host(gallery, ginv, features, table, n, budget, err, errn));
    return 0;
}

extern "C" int cp_linear_assignment_host(const double* cost, int rows, int cols, int ld, int* row_to_col)
{
    TA_FORWARD(th_linear_assignment(cost, rows, cols, ld, row_to_col, err, errn));
    return 0;
}

extern "C" int cp_track_cost_f32(const float* gallery, const float* ginv, const int* glen, const float* features, const int* slots,
                                 const float* rows, int M, int S, int Tcap, int budget, int q, float* out, void* stream)
{
    const char* who = "track_cost";
    TA_FORWARD(th_check_cost(who, M, S, Tcap, budget, q, err, errn));
    CP_CHECK_ARG(gallery && ginv && glen && features && slots && out && (rows || M == 0), "%s: null pointer", who);
    CP_CHECK_ARG(ta_aligned16(gallery), "%s: the gallery is not 16-byte aligned", who);
    CP_CHECK_ARG(ta_aligned16(features), "%s: the features are not 16-byte aligned", who);
    float* det = out + (size_t)S * Tcap * q;
    hipLaunchKernelGGL(track_cost_kernel, dim3((unsigned)(S * Tcap), (unsigned)cp_cdiv(q, TA_COLS)), dim3(TA_THREADS), 0, (hipStream_t)stream,
                       gallery, ginv, glen, features, slots, rows, M, S, Tcap, budget, q, out, det);
    CP_CHECK_LAUNCH("track_cost_kernel");
    cp_note_kernel("track_cost_kernel");
    return 0;
}

extern "C" int cp_track_append_f32(float* gallery, float* ginv, const float* features, const int* table, int n, int budget, void* stream)
{
    const char* who = "track_append";
    CP_CHECK_ARG(budget >= 1 && budget <= TH_MAX_BUDGET, "%s: budget %d outside 1..%d", who, budget, TH_MAX_BUDGET);
    CP_CHECK_ARG(n >= 0 && n <= (1 << 24), "%s: n = %d outside 0..2^24", who, n);
    CP_CHECK_ARG(gallery && ginv && features && (table || n == 0), "%s: null pointer", who);
    CP_CHECK_ARG(ta_aligned16(gallery), "%s: the gallery is not 16-byte aligned", who);
    CP_CHECK_ARG(ta_aligned16(features), "%s: the features are not 16-byte aligned", who);
    if (n == 0) return 0;
    hipLaunchKernelGGL(track_append_kernel, dim3((unsigned)n), dim3(TH_LANES), 0, (hipStream_t)stream, gallery, ginv, features, table, budget);
    CP_CHECK_LAUNCH("track_append_kernel");
    cp_note_kernel("track_append_kernel");
    return 0;
}

extern "C" int cp_track_row_ids_host(const int* slots, const int* slot_ids, int capacity, int S, int q, int M, int* row_ids)
{
    TA_FORWARD(th_row_ids_host(slots, slot_ids, capacity, S, q, M, row_ids, err, errn));
    return 0;
}

extern "C" int cp_track_row_ids(const int* slots, const int* slot_ids, int capacity, int S, int q, int M, int* row_ids, void* stream)
{
    const char* who = "track_row_ids";
    TA_FORWARD(th_check_row_ids(who, capacity, S, q, M, err, errn));
    CP_CHECK_ARG(slots && slot_ids && (row_ids || M == 0), "%s: null pointer", who);
    const int total = S * M, n = S * q;
    if (total == 0) return 0;
    hipLaunchKernelGGL(track_row_ids_fill_kernel, dim3((unsigned)cp_cdiv(total, TA_THREADS)), dim3(TA_THREADS), 0, (hipStream_t)stream, row_ids,
                       total);
    CP_CHECK_LAUNCH("track_row_ids_fill_kernel");
    hipLaunchKernelGGL(track_row_ids_scatter_kernel, dim3((unsigned)cp_cdiv(n, TA_THREADS)), dim3(TA_THREADS), 0, (hipStream_t)stream, slots,
                       slot_ids, n, total, row_ids);
    CP_CHECK_LAUNCH("track_row_ids_scatter_kernel");
    cp_note_kernel("track_row_ids_scatter_kernel");
    return 0;
}
