// draw_results: the detections of N frames painted onto those frames, in place, on the device -- the box, the 18 limbs and the 17
// joints of every row whose score is above vis_thresh (what the reference's show_results puts on the picture; its score label and
// its translucent limbs are the overlay painters of draw_overlay.hip).
// The picture is defined by draw_arith.h: integer coverage tests, painter's order, opaque stores; a frame is never read.
//
//   cp_draw_rows_frames_u8      : frames addressed by cp_frame_desc (packed / planar BGR or RGB, 3 or 4 channels, any positive strides)
//   cp_draw_rows_yuv_frames_u8  : frames addressed by cp_yuv_frame_desc (NV12 / NV21 / I420 planes), palette given as (Y, U, V)
//   cp_draw_rows_frames_host / cp_draw_rows_yuv_frames_host : the sequential HOST painters of draw_host.h, same statements
//
// Two launches per call, so nothing is handed between workgroups inside a launch:
//   1. draw_build_kernel   one wave per row; lane l < 36 builds primitive l, a ballot gives the mask of the primitives that exist and
//                          a wave reduction the row's bounding box (empty for a dead row); records go to the caller's scratch.
//   2. draw_raster_kernel  grid (tiles x, tiles y, N) sized by the largest frame, blocks beyond their own frame return.  A block walks
//                          the rows from the back in chunks of 256, compacts the rows whose bounding box meets its tile into LDS in
//                          order, and every thread looks for the last covering primitive of its pixel (YUV: of the four pixels of its
//                          2x2 block, whose chroma sample takes the winner with the highest paint index).
// Byte stores from plain C++ only.  Compiled with -ffp-contract=off like the other pre / post stages (the only float operations are
// comparisons and one float -> int conversion).
#include "common.h"
#include "draw_host.h"

#define DR_THREADS 256
#define DR_TILE 16      // a block is DR_TILE x DR_TILE threads; a thread owns one pixel (BGR) or one 2x2 block (YUV)

__global__ __launch_bounds__(DR_THREADS) void draw_build_kernel(const float* __restrict__ rows, long long total, float vis_thresh,
                                                                int box_thickness, int limb_radius, int joint_radius,
                                                                DrRowHeader* __restrict__ hdr, DaPrim* __restrict__ prims)
{
    const long long r = (long long)blockIdx.x * (DR_THREADS / CP_WAVE) + (threadIdx.x / CP_WAVE);
    if (r >= total) return;                                    // uniform over the wave
    const int lane = threadIdx.x % CP_WAVE;
    const float* row = rows + r * DA_ROW;
    DaPrim p = {0, 0, 0, 0};
    bool ok = false;
    int reach = 0;
    if (lane < DA_PRIMS && da_live(row, vis_thresh)) {
        reach = da_reach(box_thickness, limb_radius, joint_radius, lane);
        ok = reach >= 0 && da_build(row, lane, &p);
    }
    const unsigned long long mask = __ballot(ok);
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    if (ok) {
        da_bounds(p, reach, &x0, &y0, &x1, &y1);
        prims[r * DA_PRIMS + lane] = p;
    }
#pragma unroll
    for (int s = CP_WAVE / 2; s > 0; s >>= 1) {
        x0 = min(x0, __shfl_xor(x0, s)); y0 = min(y0, __shfl_xor(y0, s));
        x1 = max(x1, __shfl_xor(x1, s)); y1 = max(y1, __shfl_xor(y1, s));
    }
    if (lane == 0) hdr[r] = DrRowHeader{x0, y0, x1, y1, mask, 0};
}

// IDS: the identity-coloured form -- one more pointer and a palette, consulted only where a winner's colour is looked up
struct DrNoIds {};
template <bool IDS>
struct DrIds { typedef DrNoIds type; };
template <>
struct DrIds<true> { typedef DaIdPalette type; };

template <bool YUV, bool IDS>
__global__ __launch_bounds__(DR_THREADS) void draw_raster_kernel(const typename DrDesc<YUV>::type* __restrict__ table,
                                                                 const DrRowHeader* __restrict__ hdr, const DaPrim* __restrict__ prims, int M,
                                                                 DaStyle st, const int* __restrict__ row_ids, typename DrIds<IDS>::type idp)
{
    constexpr int S = YUV ? 2 : 1, Q = S * S;
    const typename DrDesc<YUV>::type& d = table[blockIdx.z];
    const int H = d.H, W = d.W;
    const int tx0 = blockIdx.x * (DR_TILE * S), ty0 = blockIdx.y * (DR_TILE * S);
    if (tx0 >= W || ty0 >= H) return;                          // uniform over the block
    const int tx1 = min(tx0 + DR_TILE * S, W) - 1, ty1 = min(ty0 + DR_TILE * S, H) - 1;
    const int tid = threadIdx.x, lane = tid % CP_WAVE, wave = tid / CP_WAVE;
    const int px = tx0 + (tid % DR_TILE) * S, py = ty0 + (tid / DR_TILE) * S;
    const int T = st.box_thickness, RL = st.limb_radius, RJ = st.joint_radius;
    const DrRowHeader* fh = hdr + (size_t)blockIdx.z * M;
    const DaPrim* fp = prims + (size_t)blockIdx.z * M * DA_PRIMS;

    __shared__ int list[DR_THREADS];
    __shared__ int wcount[DR_THREADS / CP_WAVE];

    int win[Q];                                                // paint index (row * 36 + primitive) of the pixel's winner, -1: none yet
    int open = 0;                                              // pixels of this thread that lie in the frame and have no winner yet
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        win[q] = -1;
        open += (px + (q % S) < W && py + (q / S) < H) ? 1 : 0;
    }

    for (int base = ((M - 1) / DR_THREADS) * DR_THREADS; base >= 0; base -= DR_THREADS) {
        const int m = base + tid;
        bool hit = false;
        if (m < M) {
            const DrRowHeader h = fh[m];
            hit = h.x0 <= tx1 && h.x1 >= tx0 && h.y0 <= ty1 && h.y1 >= ty0;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(b);
        __syncthreads();
        int before = 0, count = 0;
#pragma unroll
        for (int w = 0; w < DR_THREADS / CP_WAVE; ++w) {
            before += w < wave ? wcount[w] : 0;
            count += wcount[w];
        }
        if (hit) list[before + __popcll(b & ((1ull << lane) - 1))] = m;
        __syncthreads();
        for (int i = count - 1; i >= 0 && open > 0; --i) {
            const int r = list[i];
            const unsigned long long mask = fh[r].mask;
            const DaPrim* rp = fp + (size_t)r * DA_PRIMS;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int x = px + (q % S), y = py + (q / S);
                if (win[q] >= 0 || x >= W || y >= H) continue;
                const int l = da_row_winner(rp, mask, T, RL, RJ, x, y);
                if (l >= 0) {
                    win[q] = r * DA_PRIMS + l;
                    --open;
                }
            }
        }
        __syncthreads();                                       // the list is rewritten by the next chunk
    }

    // what the winner with paint index w stores
    auto color = [&](int w) -> const unsigned char* {
        if constexpr (IDS)
            return da_color(st, &idp, row_ids[(size_t)blockIdx.z * M + w / DA_PRIMS], w % DA_PRIMS);
        else
            return st.palette[w % DA_PRIMS];
    };

    if constexpr (YUV) {
        const DrYuvFrameDesc& f = d;
        int top = -1;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (win[q] < 0) continue;
            const int x = px + (q % S), y = py + (q / S);
            f.y_base[(long long)y * f.y_row + (long long)x * f.y_pix] = color(win[q])[0];
            top = max(top, win[q]);
        }
        if (top >= 0) {
            const long long c = (long long)(py >> 1) * f.c_row + (long long)(px >> 1) * f.c_pix;
            const unsigned char* col = color(top);
            f.u_base[c] = col[1];
            f.v_base[c] = col[2];
        }
    } else {
        const DrFrameDesc& f = d;
        if (win[0] >= 0) {
            unsigned char* p = f.base + (long long)py * f.row_stride + (long long)px * f.pix_stride;
            const unsigned char* col = color(win[0]);
#pragma unroll
            for (int k = 0; k < 3; ++k) p[f.ch_off[k]] = col[k];
        }
    }
}

extern "C" int cp_sizeof_draw_style(void) { return (int)sizeof(DaStyle); }
extern "C" size_t cp_draw_scratch_bytes(int N, int M) { return dr_scratch_bytes(N, M); }

#define DR_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" int cp_draw_rows_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style)
{
    DR_FORWARD(dr_draw_frames_host((const DrFrameDesc*)table_host, N, rows, M, vis_thresh, (const DaStyle*)style, err, errn));
    return 0;
}

extern "C" int cp_draw_rows_yuv_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style)
{
    DR_FORWARD(dr_draw_yuv_frames_host((const DrYuvFrameDesc*)table_host, N, rows, M, vis_thresh, (const DaStyle*)style, err, errn));
    return 0;
}

template <bool YUV, bool IDS>
static int dr_launch(const char* who, const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                     const DaStyle* style, void* scratch, size_t scratch_bytes, void* stream, const int* row_ids = nullptr,
                     const DaIdPalette* idp = nullptr)
{
    typedef typename DrDesc<YUV>::type Desc;
    bool noop;
    DR_FORWARD(dr_check_call(who, N, M, vis_thresh, style, &noop, err, errn));
    if (noop) return 0;
    if constexpr (IDS) DR_FORWARD(dr_check_ids(who, row_ids, idp, err, errn));
    CP_CHECK_ARG(table && table_host && rows && scratch, "%s: null pointer", who);
    CP_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    CP_CHECK_ARG(scratch_bytes >= dr_scratch_bytes(N, M), "%s: scratch of %zu bytes, %zu needed (cp_draw_scratch_bytes)", who, scratch_bytes,
                 dr_scratch_bytes(N, M));
    const Desc* th = (const Desc*)table_host;
    if constexpr (YUV) {
        DR_FORWARD(dr_check_yuv_frames(who, th, N, err, errn));
    } else {
        DR_FORWARD(dr_check_frames(who, th, N, err, errn));
    }
    int maxH = 0, maxW = 0;
    for (int n = 0; n < N; ++n) {
        if (th[n].H > maxH) maxH = th[n].H;
        if (th[n].W > maxW) maxW = th[n].W;
    }
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)N * M;
    DrRowHeader* hdr = (DrRowHeader*)scratch;
    DaPrim* prims = (DaPrim*)(hdr + total);
    const int per_block = DR_THREADS / CP_WAVE;
    hipLaunchKernelGGL(draw_build_kernel, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(DR_THREADS), 0, s, rows, total, vis_thresh,
                       style->box_thickness, style->limb_radius, style->joint_radius, hdr, prims);
    CP_CHECK_LAUNCH("draw_build_kernel");
    const int tile = DR_TILE * (YUV ? 2 : 1);
    const dim3 grid((unsigned)cp_cdiv(maxW, tile), (unsigned)cp_cdiv(maxH, tile), (unsigned)N);
    if constexpr (IDS) {
        hipLaunchKernelGGL((draw_raster_kernel<YUV, true>), grid, dim3(DR_THREADS), 0, s, (const Desc*)table, (const DrRowHeader*)hdr,
                           (const DaPrim*)prims, M, *style, row_ids, *idp);
    } else {
        hipLaunchKernelGGL((draw_raster_kernel<YUV, false>), grid, dim3(DR_THREADS), 0, s, (const Desc*)table, (const DrRowHeader*)hdr,
                           (const DaPrim*)prims, M, *style, (const int*)nullptr, DrNoIds{});
    }
    CP_CHECK_LAUNCH("draw_raster_kernel");
    if constexpr (IDS)
        cp_note_kernel(YUV ? "draw_raster_kernel<yuv,ids>" : "draw_raster_kernel<bgr,ids>");
    else
        cp_note_kernel(YUV ? "draw_raster_kernel<yuv>" : "draw_raster_kernel<bgr>");
    return 0;
}

extern "C" int cp_draw_rows_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                      const void* style, void* scratch, size_t scratch_bytes, void* stream)
{
    return dr_launch<false, false>("draw_rows_frames", table, table_host, N, rows, M, vis_thresh, (const DaStyle*)style, scratch, scratch_bytes,
                                   stream);
}

extern "C" int cp_draw_rows_yuv_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                          const void* style, void* scratch, size_t scratch_bytes, void* stream)
{
    return dr_launch<true, false>("draw_rows_yuv_frames", table, table_host, N, rows, M, vis_thresh, (const DaStyle*)style, scratch, scratch_bytes,
                                  stream);
}

// the identity-coloured forms: the same launches with row_ids DEVICE int [N, M] and a HOST cp_draw_id_palette
extern "C" int cp_draw_rows_ids_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                          const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                                          void* stream)
{
    return dr_launch<false, true>("draw_rows_ids_frames", table, table_host, N, rows, M, vis_thresh, (const DaStyle*)style, scratch,
                                  scratch_bytes, stream, row_ids, (const DaIdPalette*)id_palette);
}

extern "C" int cp_draw_rows_ids_yuv_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                              const void* style, void* scratch, size_t scratch_bytes, const int* row_ids,
                                              const void* id_palette, void* stream)
{
    return dr_launch<true, true>("draw_rows_ids_yuv_frames", table, table_host, N, rows, M, vis_thresh, (const DaStyle*)style, scratch,
                                 scratch_bytes, stream, row_ids, (const DaIdPalette*)id_palette);
}

extern "C" int cp_draw_rows_ids_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                            const int* row_ids, const void* id_palette)
{
    DR_FORWARD(dr_draw_frames_host((const DrFrameDesc*)table_host, N, rows, M, vis_thresh, (const DaStyle*)style, err, errn, true, row_ids,
                                   (const DaIdPalette*)id_palette));
    return 0;
}

extern "C" int cp_draw_rows_ids_yuv_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                                const int* row_ids, const void* id_palette)
{
    DR_FORWARD(dr_draw_yuv_frames_host((const DrYuvFrameDesc*)table_host, N, rows, M, vis_thresh, (const DaStyle*)style, err, errn, true, row_ids,
                                       (const DaIdPalette*)id_palette));
    return 0;
}
