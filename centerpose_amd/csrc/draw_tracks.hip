// draw_tracks: the tracks of N frames painted onto those frames, in place, on the device -- per track its box in the track's colour, a
// filled bar at the box's top-left corner and the label written on the bar in the library's 5 x 7 font (what the reference's
// draw_bboxes puts on the picture).  The picture is defined by draw_text_arith.h: integer coverage tests, painter's order, opaque
// stores; a frame is never read.
//
//   cp_draw_tracks_frames_u8      : frames addressed by cp_frame_desc (packed / planar BGR or RGB, 3 or 4 channels, any positive strides)
//   cp_draw_tracks_yuv_frames_u8  : frames addressed by cp_yuv_frame_desc (NV12 / NV21 / I420 planes), item colours given as (Y, U, V)
//   cp_draw_tracks_frames_host / cp_draw_tracks_yuv_frames_host : the sequential HOST painters of draw_tracks_host.h, same statements
//   cp_draw_glyph_rows            : the font, one glyph at a time
//
// Tracks are host data, so the caller uploads the finished item table: there is no build launch.  One launch per call:
//   draw_tracks_kernel  grid (tiles x, tiles y, N) sized by the largest frame, blocks beyond their own frame return.  A block walks
//                       its frame's items from the back in chunks of 256, compacts the items whose bounding box (box and bar) meets
//                       its tile into LDS in order, and every thread looks for the last covering primitive of its pixel, text before
//                       bar before box (YUV: of the four pixels of its 2x2 block, whose chroma sample takes the winner with the
//                       highest paint index).
// Byte stores from plain C++ only.  No float operation at all.
#include "common.h"
#include "draw_tracks_host.h"

#define DK_THREADS 256
#define DK_TILE 16      // a block is DK_TILE x DK_TILE threads; a thread owns one pixel (BGR) or one 2x2 block (YUV)

template <bool YUV>
__global__ __launch_bounds__(DK_THREADS) void draw_tracks_kernel(const typename DrDesc<YUV>::type* __restrict__ table,
                                                                 const DtItem* __restrict__ items, const int* __restrict__ counts, int Kmax,
                                                                 int T, int s)
{
    constexpr int S = YUV ? 2 : 1, Q = S * S;
    const typename DrDesc<YUV>::type& d = table[blockIdx.z];
    const int H = d.H, W = d.W;
    const int tx0 = blockIdx.x * (DK_TILE * S), ty0 = blockIdx.y * (DK_TILE * S);
    if (tx0 >= W || ty0 >= H) return;                          // uniform over the block
    const int tx1 = min(tx0 + DK_TILE * S, W) - 1, ty1 = min(ty0 + DK_TILE * S, H) - 1;
    const int tid = threadIdx.x, lane = tid % CP_WAVE, wave = tid / CP_WAVE;
    const int px = tx0 + (tid % DK_TILE) * S, py = ty0 + (tid / DK_TILE) * S;
    const DtItem* fi = items + (size_t)blockIdx.z * Kmax;
    const int K = min(max(counts[blockIdx.z], 0), Kmax);       // the launcher refused a count outside 0..Kmax on the host copy

    __shared__ int list[DK_THREADS];
    __shared__ int wcount[DK_THREADS / CP_WAVE];

    int win[Q];                                                // paint index (item * 3 + primitive) of the pixel's winner, -1: none yet
    int open = 0;                                              // pixels of this thread that lie in the frame and have no winner yet
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        win[q] = -1;
        open += (px + (q % S) < W && py + (q / S) < H) ? 1 : 0;
    }

    for (int base = K > 0 ? ((K - 1) / DK_THREADS) * DK_THREADS : -1; base >= 0; base -= DK_THREADS) {
        const int k = base + tid;
        bool hit = false;
        if (k < K) {
            int x0, y0, x1, y1;
            dt_bounds(fi[k], s, &x0, &y0, &x1, &y1);
            hit = x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(b);
        __syncthreads();
        int before = 0, count = 0;
#pragma unroll
        for (int w = 0; w < DK_THREADS / CP_WAVE; ++w) {
            before += w < wave ? wcount[w] : 0;
            count += wcount[w];
        }
        if (hit) list[before + __popcll(b & ((1ull << lane) - 1))] = k;
        __syncthreads();
        for (int i = count - 1; i >= 0 && open > 0; --i) {
            const int r = list[i];
            const DtItem& it = fi[r];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int x = px + (q % S), y = py + (q / S);
                if (win[q] >= 0 || x >= W || y >= H) continue;
                const int l = dt_item_winner(it, T, s, x, y);
                if (l >= 0) {
                    win[q] = r * DT_PRIMS + l;
                    --open;
                }
            }
        }
        __syncthreads();                                       // the list is rewritten by the next chunk
    }

    if constexpr (YUV) {
        const DrYuvFrameDesc& f = d;
        int top = -1;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (win[q] < 0) continue;
            const int x = px + (q % S), y = py + (q / S);
            const DtItem& it = fi[win[q] / DT_PRIMS];
            f.y_base[(long long)y * f.y_row + (long long)x * f.y_pix] = (win[q] % DT_PRIMS == 2 ? it.text_color : it.color)[0];
            top = max(top, win[q]);
        }
        if (top >= 0) {
            const DtItem& it = fi[top / DT_PRIMS];
            const unsigned char* c = top % DT_PRIMS == 2 ? it.text_color : it.color;
            const long long o = (long long)(py >> 1) * f.c_row + (long long)(px >> 1) * f.c_pix;
            f.u_base[o] = c[1];
            f.v_base[o] = c[2];
        }
    } else {
        const DrFrameDesc& f = d;
        if (win[0] >= 0) {
            unsigned char* p = f.base + (long long)py * f.row_stride + (long long)px * f.pix_stride;
            const DtItem& it = fi[win[0] / DT_PRIMS];
            const unsigned char* c = win[0] % DT_PRIMS == 2 ? it.text_color : it.color;
#pragma unroll
            for (int j = 0; j < 3; ++j) p[f.ch_off[j]] = c[j];
        }
    }
}

extern "C" int cp_sizeof_draw_track_item(void) { return (int)sizeof(DtItem); }

extern "C" int cp_draw_glyph_rows(int ch, unsigned char* rows)
{
    const int g = dt_glyph_index(ch);
    if (g < 0 || !rows) return -1;
    for (int r = 0; r < DT_GLYPH_ROWS; ++r) rows[r] = (unsigned char)dt_font_row(g, r);
    return g;
}

#define DK_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" int cp_draw_tracks_frames_host(const void* table_host, int N, const void* items, const int* counts, int Kmax, int box_thickness,
                                          int font_scale)
{
    DK_FORWARD(dk_draw_frames_host((const DrFrameDesc*)table_host, N, (const DtItem*)items, counts, Kmax, box_thickness, font_scale, err, errn));
    return 0;
}

extern "C" int cp_draw_tracks_yuv_frames_host(const void* table_host, int N, const void* items, const int* counts, int Kmax,
                                              int box_thickness, int font_scale)
{
    DK_FORWARD(dk_draw_yuv_frames_host((const DrYuvFrameDesc*)table_host, N, (const DtItem*)items, counts, Kmax, box_thickness, font_scale, err,
                                       errn));
    return 0;
}

template <bool YUV>
static int dk_launch(const char* who, const void* table, const void* table_host, int N, const void* items, const void* items_host,
                     const int* counts, const int* counts_host, int Kmax, int T, int s, void* stream)
{
    typedef typename DrDesc<YUV>::type Desc;
    bool noop;
    long long total;
    DK_FORWARD(dk_check_call(who, N, Kmax, T, s, &noop, err, errn));
    if (noop) return 0;
    CP_CHECK_ARG(table && table_host && items && items_host && counts && counts_host, "%s: null pointer", who);
    CP_CHECK_ARG(((uintptr_t)items & 3) == 0 && ((uintptr_t)counts & 3) == 0, "%s: items and counts must be 4-byte aligned", who);
    DK_FORWARD(dk_check_items(who, (const DtItem*)items_host, counts_host, N, Kmax, &total, err, errn));
    const Desc* th = (const Desc*)table_host;
    if constexpr (YUV) {
        DK_FORWARD(dr_check_yuv_frames(who, th, N, err, errn));
    } else {
        DK_FORWARD(dr_check_frames(who, th, N, err, errn));
    }
    if (total == 0) return 0;                                  // no items: nothing is launched
    int maxH = 0, maxW = 0;
    for (int n = 0; n < N; ++n) {
        if (th[n].H > maxH) maxH = th[n].H;
        if (th[n].W > maxW) maxW = th[n].W;
    }
    const int tile = DK_TILE * (YUV ? 2 : 1);
    hipLaunchKernelGGL(draw_tracks_kernel<YUV>, dim3((unsigned)cp_cdiv(maxW, tile), (unsigned)cp_cdiv(maxH, tile), (unsigned)N), dim3(DK_THREADS), 0,
                       (hipStream_t)stream, (const Desc*)table, (const DtItem*)items, counts, Kmax, T, s);
    CP_CHECK_LAUNCH("draw_tracks_kernel");
    cp_note_kernel(YUV ? "draw_tracks_kernel<yuv>" : "draw_tracks_kernel<bgr>");
    return 0;
}

extern "C" int cp_draw_tracks_frames_u8(const void* table, const void* table_host, int N, const void* items, const void* items_host,
                                        const int* counts, const int* counts_host, int Kmax, int box_thickness, int font_scale, void* stream)
{
    return dk_launch<false>("draw_tracks_frames", table, table_host, N, items, items_host, counts, counts_host, Kmax, box_thickness, font_scale,
                            stream);
}

extern "C" int cp_draw_tracks_yuv_frames_u8(const void* table, const void* table_host, int N, const void* items, const void* items_host,
                                            const int* counts, const int* counts_host, int Kmax, int box_thickness, int font_scale,
                                            void* stream)
{
    return dk_launch<true>("draw_tracks_yuv_frames", table, table_host, N, items, items_host, counts, counts_host, Kmax, box_thickness, font_scale,
                           stream);
}
