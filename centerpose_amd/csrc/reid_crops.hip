// Re-id crops: the detections of N device frames cut out of those frames, resized to 3 x 128 x 64 and normalised, straight into the
// input tensor of the re-id plan -- what DeepSort._get_features + Extractor._preprocess do per box on the host
// (demo/tracking/deep_sort.py:75-86, feature_extractor.py:24-39), for all boxes of all frames in two launches.  The values are
// defined by reid_arith.h; the frames are read where they lie, never written.
//
//   cp_reid_select_rows           : which rows get an embedding and in which slot (one wave per frame, ballot + prefix count)
//   cp_reid_crop_frames_f32       : frames addressed by cp_frame_desc (packed / planar BGR or RGB, 3 or 4 channels, any strides)
//   cp_reid_crop_yuv_frames_f32   : frames addressed by cp_yuv_frame_desc (NV12 / NV21 / I420), converted per source pixel; a table with
//                                   any non-zero format word (yuv_source.h: P010 / P016, 4:2:2, 4:4:4, grey) runs the general
//                                   instantiation, reid_crop_kernel<surfaces>
//   cp_reid_*_host                : the sequential HOST twins of reid_host.h, same statements
//
// The crop kernel is a gather: blockIdx.y is the slot, a thread owns one output pixel, consecutive lanes consecutive ox, so a wave
// stores one whole 64-float row (256 contiguous bytes) per channel plane and its taps fall on neighbouring source bytes.  64-bit
// addressing throughout.  Compiled with -ffp-contract=off.
#include "common.h"
#include "reid_host.h"

#define RC_THREADS 256

template <bool YUV>
struct RcDesc { typedef RhFrameDesc type; };
template <>
struct RcDesc<true> { typedef RhYuvFrameDesc type; };

// grid N, one wave each.  The wave walks its frame's M rows 64 at a time; a ballot of the selected lanes and the count so far give
// every selected row its rank, the first q of them their slot.  The wave then marks its unused slots, and the last frame's wave the
// slots beyond N * q.
template <bool YUV>
__global__ __launch_bounds__(CP_WAVE) void reid_select_kernel(const typename RcDesc<YUV>::type* __restrict__ table, int N,
                                                              const float* __restrict__ rows, int M, float vis_thresh, int cap,
                                                              int* __restrict__ slots, int* __restrict__ counts)
{
    const int n = blockIdx.x, lane = threadIdx.x, q = cap / N;
    const int H = table[n].H, W = table[n].W;
    int count = 0;
    for (int base = 0; base < M; base += CP_WAVE) {
        const int m = base + lane;
        bool sel = false;
        if (m < M) {
            RaBox b;
            sel = ra_select(rows + ((size_t)n * M + m) * RA_ROW, vis_thresh, H, W, &b);
        }
        const unsigned long long mask = __ballot(sel);
        const int rank = count + __popcll(mask & ((1ull << lane) - 1));
        if (sel && rank < q) slots[n * q + rank] = n * M + m;
        count += __popcll(mask);
    }
    for (int s = (count < q ? count : q) + lane; s < q; s += CP_WAVE) slots[n * q + s] = -1;
    if (n == N - 1)
        for (int s = N * q + lane; s < cap; s += CP_WAVE) slots[s] = -1;
    if (lane == 0) counts[n] = count;
}

// grid (128 * 64 / 256, cap).  GEN (YUV only): the sampler reads the frame's format word; false: every frame is 8-bit 4:2:0
template <bool YUV, bool GEN>
__global__ __launch_bounds__(RC_THREADS) void reid_crop_kernel(const typename RcDesc<YUV>::type* __restrict__ table, int N,
                                                               const float* __restrict__ rows, int M, float vis_thresh,
                                                               const int* __restrict__ slots, YfCoef coef, RaNorm nm, float* __restrict__ out)
{
    const int s = blockIdx.y, p = blockIdx.x * RC_THREADS + threadIdx.x;       // p < 128 * 64: the grid is exact
    const int oy = p / RA_OUT_W, ox = p % RA_OUT_W;
    const size_t plane = (size_t)RA_OUT_H * RA_OUT_W;
    float* o = out + (size_t)s * 3 * plane + p;
    const int idx = slots[s];                                                   // uniform over the block
    float r[3] = {0.f, 0.f, 0.f};
    RaBox b;
    if (idx >= 0 && idx < N * M && ra_select(rows + (size_t)idx * RA_ROW, vis_thresh, table[idx / M].H, table[idx / M].W, &b)) {
        const typename RcDesc<YUV>::type& d = table[idx / M];
        if constexpr (YUV)
            ra_pixel(rh_yuv_source<GEN>(d, coef), b, oy, ox, nm, r);
        else
            ra_pixel(rh_source(d), b, oy, ox, nm, r);
    }
    o[0] = r[0];
    o[plane] = r[1];
    o[2 * plane] = r[2];
}

#define RC_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" int cp_sizeof_reid_norm(void) { return (int)sizeof(RaNorm); }

extern "C" int cp_reid_select_rows_host(const void* table_host, int yuv, int N, const float* rows, int M, float vis_thresh, int cap,
                                        int* slots, int* counts)
{
    RC_FORWARD(rh_select_host(table_host, yuv, N, rows, M, vis_thresh, cap, slots, counts, err, errn));
    return 0;
}

extern "C" int cp_reid_crop_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const int* slots, int cap,
                                        const void* norm, float* out)
{
    RC_FORWARD(rh_crop_frames_host((const RhFrameDesc*)table_host, N, rows, M, vis_thresh, slots, cap, (const RaNorm*)norm, out, err, errn));
    return 0;
}

extern "C" int cp_reid_crop_yuv_frames_host(const void* table_host, int N, const int* coef, const float* rows, int M, float vis_thresh,
                                            const int* slots, int cap, const void* norm, float* out)
{
    RC_FORWARD(rh_crop_yuv_frames_host((const RhYuvFrameDesc*)table_host, N, coef, rows, M, vis_thresh, slots, cap, (const RaNorm*)norm, out,
                                       err, errn));
    return 0;
}

// Only H and W of a descriptor are read here; they are checked to be positive (a crop launch checks the addressing fields).
extern "C" int cp_reid_select_rows(const void* table, const void* table_host, int yuv, int N, const float* rows, int M, float vis_thresh,
                                   int cap, int* slots, int* counts, void* stream)
{
    const char* who = "reid_select_rows";
    RC_FORWARD(rh_check_call(who, N, M, cap, err, errn));
    CP_CHECK_ARG(table && table_host && slots && counts && (rows || M == 0), "%s: null pointer", who);
    for (int n = 0; n < N; ++n) {
        const int H = yuv ? ((const RhYuvFrameDesc*)table_host)[n].H : ((const RhFrameDesc*)table_host)[n].H;
        const int W = yuv ? ((const RhYuvFrameDesc*)table_host)[n].W : ((const RhFrameDesc*)table_host)[n].W;
        CP_CHECK_ARG(H > 0 && W > 0 && (long long)H * W < (1ll << 29), "%s: frame %d: bad size %d x %d", who, n, H, W);
    }
    if (yuv) RC_FORWARD(rh_check_yuv_words(who, (const RhYuvFrameDesc*)table_host, N, err, errn));
    if (yuv)
        hipLaunchKernelGGL(reid_select_kernel<true>, dim3((unsigned)N), dim3(CP_WAVE), 0, (hipStream_t)stream, (const RhYuvFrameDesc*)table, N,
                           rows, M, vis_thresh, cap, slots, counts);
    else
        hipLaunchKernelGGL(reid_select_kernel<false>, dim3((unsigned)N), dim3(CP_WAVE), 0, (hipStream_t)stream, (const RhFrameDesc*)table, N,
                           rows, M, vis_thresh, cap, slots, counts);
    CP_CHECK_LAUNCH("reid_select_kernel");
    cp_note_kernel(yuv ? "reid_select_kernel<yuv>" : "reid_select_kernel<bgr>");
    return 0;
}

template <bool YUV>
static int rc_launch(const char* who, const void* table, const void* table_host, int N, const int* coef, const float* rows, int M,
                     float vis_thresh, const int* slots, int cap, const RaNorm* nm, float* out, void* stream)
{
    typedef typename RcDesc<YUV>::type Desc;
    RC_FORWARD(rh_check_call(who, N, M, cap, err, errn));
    RC_FORWARD(rh_check_norm(who, nm, err, errn));
    CP_CHECK_ARG(table && table_host && slots && out && (rows || M == 0), "%s: null pointer", who);
    YfCoef k = {0, 0, 0, 0, 0, 0};
    bool general = false;
    if constexpr (YUV) {
        RC_FORWARD(rh_check_yuv_frames(who, (const Desc*)table_host, N, coef, err, errn));
        k = YfCoef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
        for (int n = 0; n < N; ++n) general = general || ((const Desc*)table_host)[n].pad != 0;
    } else {
        RC_FORWARD(rh_check_frames(who, (const Desc*)table_host, N, err, errn));
    }
    static_assert((RA_OUT_H * RA_OUT_W) % RC_THREADS == 0, "the crop grid is exact");
    const dim3 grid(RA_OUT_H * RA_OUT_W / RC_THREADS, (unsigned)cap);
    if (general)
        hipLaunchKernelGGL((reid_crop_kernel<YUV, YUV>), grid, dim3(RC_THREADS), 0, (hipStream_t)stream, (const Desc*)table, N, rows, M, vis_thresh,
                           slots, k, *nm, out);
    else
        hipLaunchKernelGGL((reid_crop_kernel<YUV, false>), grid, dim3(RC_THREADS), 0, (hipStream_t)stream, (const Desc*)table, N, rows, M, vis_thresh,
                           slots, k, *nm, out);
    CP_CHECK_LAUNCH("reid_crop_kernel");
    cp_note_kernel(general ? "reid_crop_kernel<surfaces>" : YUV ? "reid_crop_kernel<yuv>" : "reid_crop_kernel<bgr>");
    return 0;
}

extern "C" int cp_reid_crop_frames_f32(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                       const int* slots, int cap, const void* norm, float* out, void* stream)
{
    return rc_launch<false>("reid_crop_frames", table, table_host, N, nullptr, rows, M, vis_thresh, slots, cap, (const RaNorm*)norm, out, stream);
}

extern "C" int cp_reid_crop_yuv_frames_f32(const void* table, const void* table_host, int N, const int* coef, const float* rows, int M,
                                           float vis_thresh, const int* slots, int cap, const void* norm, float* out, void* stream)
{
    return rc_launch<true>("reid_crop_yuv_frames", table, table_host, N, coef, rows, M, vis_thresh, slots, cap, (const RaNorm*)norm, out, stream);
}
