// 3-D face alignment for detections, the stages around the PRNet plan: the faces of N device frames cut out of those frames by a
// similarity crop to 3 x 256 x 256, straight into the input tensor of the plan, and the plan's position maps taken back to image
// coordinates with their 68 landmarks -- what PRN.process and PRN.get_landmarks do per face on the host (demo/face/prnet.py:61-127),
// for all faces of all frames in three launches.  The values are defined by face_arith.h (a closed-form statement of that pipeline,
// not pinned to a recording of skimage); the frames are read where they lie, never written.
//
//   cp_face_select                 : which candidates (detection rows or given boxes) get a crop, in which slot, with which square
//                                    (one wave per frame, ballot + prefix count)
//   cp_face_crop_frames_f32        : frames addressed by cp_frame_desc (packed / planar BGR or RGB, 3 or 4 channels, any strides)
//   cp_face_crop_yuv_frames_f32    : frames addressed by cp_yuv_frame_desc; a table with any non-zero format word (yuv_source.h) runs
//                                    the general instantiation, face_crop_kernel<surfaces>
//   cp_face_restore_f32            : position maps and landmarks in image coordinates
//   cp_face_*_host                 : the sequential HOST twins of face_host.h, same statements
//
// The crop kernel is a gather: blockIdx.y is the slot, a thread owns one output pixel, consecutive lanes consecutive columns, so a
// wave stores 256 contiguous bytes per channel plane and its taps fall on neighbouring source bytes.  64-bit addressing throughout.
// Compiled with -ffp-contract=off.
#include "common.h"
#include "face_host.h"

#define FC_THREADS 256

template <bool YUV>
struct FcDesc { typedef RhFrameDesc type; };
template <>
struct FcDesc<true> { typedef RhYuvFrameDesc type; };

// grid N, one wave each.  The wave walks its frame's M candidates 64 at a time; a ballot of the selected lanes and the count so far
// give every selected candidate its rank, the first q of them their slot.  The wave then marks its unused slots, and the last frame's
// wave the slots beyond N * q.
__global__ __launch_bounds__(CP_WAVE) void face_select_kernel(int N, const float* __restrict__ cand, int M, FhRule rule, int cap,
                                                              int* __restrict__ slots, int* __restrict__ counts, float* __restrict__ xform)
{
    const int n = blockIdx.x, lane = threadIdx.x, q = cap / N, stride = rule.boxes ? FA_BOX : FA_ROW;
    int count = 0;
    for (int base = 0; base < M; base += CP_WAVE) {
        const int m = base + lane;
        bool sel = false;
        FaXform t = {0.f, 0.f, 0.f};
        if (m < M) sel = fa_select(cand + ((size_t)n * M + m) * stride, rule.boxes, rule.vis_thresh, rule.expand, rule.min_size, &t);
        const unsigned long long mask = __ballot(sel);
        const int rank = count + __popcll(mask & ((1ull << lane) - 1));
        if (sel && rank < q) {
            const int s = n * q + rank;
            slots[s] = n * M + m;
            xform[3 * s] = t.x0; xform[3 * s + 1] = t.y0; xform[3 * s + 2] = t.size;
        }
        count += __popcll(mask);
    }
    for (int s = (count < q ? count : q) + lane; s < q; s += CP_WAVE) {
        slots[n * q + s] = -1;
        xform[3 * (n * q + s)] = 0.f; xform[3 * (n * q + s) + 1] = 0.f; xform[3 * (n * q + s) + 2] = 0.f;
    }
    if (n == N - 1)
        for (int s = N * q + lane; s < cap; s += CP_WAVE) {
            slots[s] = -1;
            xform[3 * s] = 0.f; xform[3 * s + 1] = 0.f; xform[3 * s + 2] = 0.f;
        }
    if (lane == 0) counts[n] = count;
}

// grid (256 * 256 / 256, cap).  GEN (YUV only): the sampler reads the frame's format word; false: every frame is 8-bit 4:2:0
template <bool YUV, bool GEN>
__global__ __launch_bounds__(FC_THREADS) void face_crop_kernel(const typename FcDesc<YUV>::type* __restrict__ table, int N, int M,
                                                               const int* __restrict__ slots, const float* __restrict__ xform, YfCoef coef,
                                                               float* __restrict__ out)
{
    const int s = blockIdx.y, p = blockIdx.x * FC_THREADS + threadIdx.x;       // p < 256 * 256: the grid is exact
    const int v = p / FA_RES, u = p % FA_RES;
    const size_t plane = (size_t)FA_RES * FA_RES;
    float* o = out + (size_t)s * 3 * plane + p;
    float r[3] = {0.f, 0.f, 0.f};
    FaXform t;
    if (fh_slot(slots, xform, s, N, M, &t)) {                                   // uniform over the block
        const typename FcDesc<YUV>::type& d = table[slots[s] / M];
        if constexpr (YUV)
            fa_pixel(rh_yuv_source<GEN>(d, coef), d.H, d.W, t, v, u, r);
        else
            fa_pixel(rh_source(d), d.H, d.W, t, v, u, r);
    }
    o[0] = r[0];
    o[plane] = r[1];
    o[2 * plane] = r[2];
}

// grid (256 * 256 / 256, cap): the whole map, a thread per cell (three planar loads, twelve contiguous bytes stored)
__global__ __launch_bounds__(FC_THREADS) void face_restore_map_kernel(const float* __restrict__ net, const int* __restrict__ slots,
                                                                      const float* __restrict__ xform, float* __restrict__ pos)
{
    const int s = blockIdx.y;
    const size_t plane = (size_t)FA_RES * FA_RES, c = (size_t)blockIdx.x * FC_THREADS + threadIdx.x;
    const float* o = net + (size_t)s * 3 * plane;
    float r[3] = {0.f, 0.f, 0.f};
    FaXform t;
    if (fh_slot(slots, xform, s, 1, FA_MAX_ROWS, &t)) fa_restore(t, o[c], o[plane + c], o[2 * plane + c], r);
    float* w = pos + ((size_t)s * plane + c) * 3;
    w[0] = r[0]; w[1] = r[1]; w[2] = r[2];
}

// grid cap, 128 threads: the 68 landmark cells of a slot
__global__ __launch_bounds__(128) void face_landmarks_kernel(const float* __restrict__ net, const int* __restrict__ slots,
                                                             const float* __restrict__ xform, const int* __restrict__ uv,
                                                             float* __restrict__ landmarks)
{
    const int s = blockIdx.x, j = threadIdx.x;
    if (j >= FA_NKPT) return;
    const size_t plane = (size_t)FA_RES * FA_RES;
    const int col = uv[j], row = uv[FA_NKPT + j];
    float r[3] = {0.f, 0.f, 0.f};
    FaXform t;
    if (fh_slot(slots, xform, s, 1, FA_MAX_ROWS, &t) && col >= 0 && col < FA_RES && row >= 0 && row < FA_RES) {
        const float* o = net + (size_t)s * 3 * plane + (size_t)row * FA_RES + col;
        fa_restore(t, o[0], o[plane], o[2 * plane], r);
    }
    float* w = landmarks + ((size_t)s * FA_NKPT + j) * 3;
    w[0] = r[0]; w[1] = r[1]; w[2] = r[2];
}

#define FC_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" int cp_sizeof_face_rule(void) { return (int)sizeof(FhRule); }

extern "C" int cp_face_select_host(int N, const float* cand, int M, const void* rule, int cap, int* slots, int* counts, float* xform)
{
    FC_FORWARD(fh_select_host(N, cand, M, (const FhRule*)rule, cap, slots, counts, xform, err, errn));
    return 0;
}

extern "C" int cp_face_crop_frames_host(const void* table_host, int N, int M, const int* slots, const float* xform, int cap, float* out)
{
    FC_FORWARD(fh_crop_frames_host((const RhFrameDesc*)table_host, N, M, slots, xform, cap, out, err, errn));
    return 0;
}

extern "C" int cp_face_crop_yuv_frames_host(const void* table_host, int N, const int* coef, int M, const int* slots, const float* xform,
                                            int cap, float* out)
{
    FC_FORWARD(fh_crop_yuv_frames_host((const RhYuvFrameDesc*)table_host, N, coef, M, slots, xform, cap, out, err, errn));
    return 0;
}

extern "C" int cp_face_restore_host(const float* net, const int* slots, const float* xform, int cap, const int* uv, float* pos,
                                    float* landmarks)
{
    FC_FORWARD(fh_restore_host(net, slots, xform, cap, uv, pos, landmarks, err, errn));
    return 0;
}

extern "C" int cp_face_select(int N, const float* cand, int M, const void* rule, int cap, int* slots, int* counts, float* xform,
                              void* stream)
{
    const char* who = "face_select";
    FC_FORWARD(fh_check_call(who, N, M, cap, err, errn));
    FC_FORWARD(fh_check_rule(who, (const FhRule*)rule, err, errn));
    CP_CHECK_ARG(slots && counts && xform && (cand || M == 0), "%s: null pointer", who);
    hipLaunchKernelGGL(face_select_kernel, dim3((unsigned)N), dim3(CP_WAVE), 0, (hipStream_t)stream, N, cand, M, *(const FhRule*)rule, cap,
                       slots, counts, xform);
    CP_CHECK_LAUNCH("face_select_kernel");
    cp_note_kernel(((const FhRule*)rule)->boxes ? "face_select_kernel<boxes>" : "face_select_kernel<rows>");
    return 0;
}

template <bool YUV>
static int fc_launch(const char* who, const void* table, const void* table_host, int N, const int* coef, int M, const int* slots,
                     const float* xform, int cap, float* out, void* stream)
{
    typedef typename FcDesc<YUV>::type Desc;
    FC_FORWARD(fh_check_call(who, N, M, cap, err, errn));
    CP_CHECK_ARG(table && table_host && slots && xform && out, "%s: null pointer", who);
    YfCoef k = {0, 0, 0, 0, 0, 0};
    bool general = false;
    if constexpr (YUV) {
        FC_FORWARD(rh_check_yuv_frames(who, (const Desc*)table_host, N, coef, err, errn));
        k = YfCoef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
        for (int n = 0; n < N; ++n) general = general || ((const Desc*)table_host)[n].pad != 0;
    } else {
        FC_FORWARD(rh_check_frames(who, (const Desc*)table_host, N, err, errn));
    }
    static_assert((FA_RES * FA_RES) % FC_THREADS == 0, "the crop grid is exact");
    const dim3 grid(FA_RES * FA_RES / FC_THREADS, (unsigned)cap);
    if (general)
        hipLaunchKernelGGL((face_crop_kernel<YUV, YUV>), grid, dim3(FC_THREADS), 0, (hipStream_t)stream, (const Desc*)table, N, M, slots, xform, k,
                           out);
    else
        hipLaunchKernelGGL((face_crop_kernel<YUV, false>), grid, dim3(FC_THREADS), 0, (hipStream_t)stream, (const Desc*)table, N, M, slots, xform,
                           k, out);
    CP_CHECK_LAUNCH("face_crop_kernel");
    cp_note_kernel(general ? "face_crop_kernel<surfaces>" : YUV ? "face_crop_kernel<yuv>" : "face_crop_kernel<bgr>");
    return 0;
}

extern "C" int cp_face_crop_frames_f32(const void* table, const void* table_host, int N, int M, const int* slots, const float* xform, int cap,
                                       float* out, void* stream)
{
    return fc_launch<false>("face_crop_frames", table, table_host, N, nullptr, M, slots, xform, cap, out, stream);
}

extern "C" int cp_face_crop_yuv_frames_f32(const void* table, const void* table_host, int N, const int* coef, int M, const int* slots,
                                           const float* xform, int cap, float* out, void* stream)
{
    return fc_launch<true>("face_crop_yuv_frames", table, table_host, N, coef, M, slots, xform, cap, out, stream);
}

// uv DEVICE int [2][68], checked by the caller (face.FaceAligner) when it is uploaded; a cell outside the map gives a zero landmark.
// pos may be null: the 68 points only, the map is never written.
extern "C" int cp_face_restore_f32(const float* net, const int* slots, const float* xform, int cap, const int* uv, float* pos,
                                   float* landmarks, void* stream)
{
    const char* who = "face_restore";
    CP_CHECK_ARG(cap >= 1 && cap <= FA_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FA_MAX_CAP);
    CP_CHECK_ARG(net && slots && xform && uv && landmarks, "%s: null pointer", who);
    if (pos) {
        hipLaunchKernelGGL(face_restore_map_kernel, dim3(FA_RES * FA_RES / FC_THREADS, (unsigned)cap), dim3(FC_THREADS), 0, (hipStream_t)stream,
                           net, slots, xform, pos);
        CP_CHECK_LAUNCH("face_restore_map_kernel");
    }
    hipLaunchKernelGGL(face_landmarks_kernel, dim3((unsigned)cap), dim3(128), 0, (hipStream_t)stream, net, slots, xform, uv, landmarks);
    CP_CHECK_LAUNCH("face_landmarks_kernel");
    cp_note_kernel(pos ? "face_restore_map_kernel+face_landmarks_kernel" : "face_landmarks_kernel");
    return 0;
}
