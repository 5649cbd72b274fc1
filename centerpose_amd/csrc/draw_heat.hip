// draw_heat: the network's heat maps blended over N device frames, in place -- the reference's debug views pred_hm / pred_hmhp
// (MultiPoseDetector.debug: Debugger.gen_colormap / gen_colormap_hp, add_blend_img).  The picture is defined by draw_heat_arith.h: a
// colour map per image (the per-component maximum of value x channel colour), sampled bilinearly in fixed point at the map position of
// every frame pixel, and an integer blend.  Unlike the primitive painters this one reads and writes EVERY pixel of every frame.
//
//   cp_draw_heat_frames_u8      : frames addressed by cp_frame_desc (packed / planar BGR or RGB, 3 or 4 channels, any positive strides)
//   cp_draw_heat_yuv_frames_u8  : frames addressed by cp_yuv_frame_desc (NV12 / NV21 / I420 planes)
//   cp_draw_heat_frames_host / cp_draw_heat_yuv_frames_host : the sequential HOST painters of draw_heat_host.h, same statements
//   cp_bgr_to_yuv_host          : the forward colour form of the YUV painters, over an array
//
// Two launches per call, nothing is handed between workgroups inside a launch:
//   1. draw_heat_colormap_kernel          one thread per image and map cell: a loop over the C channels through the maps' four element
//                                         strides (the maps are never copied), one dword stored.
//   2. draw_heat_blend_kernel<bgr>        one pixel per thread, byte loads and stores: any strides, planar layouts, 4-channel frames.
//      draw_heat_blend_kernel<bgr_packed> hwc frames with pixel stride 3 (every frame of the call): a thread owns four consecutive pixels
//                                         whose first byte is 4-byte aligned and loads and stores their 12 bytes as three dwords -- every
//                                         stored byte is a colour byte of a pixel of the view; the up to three pixels before the first
//                                         aligned one and the up to three after the last whole group of a row go through byte accesses
//                                         of further threads of the same launch.  Bit-identical to <bgr>.
//      draw_heat_blend_kernel<yuv>        one 2x2 block with its chroma sample per thread, byte loads and stores.
//    A block is 64 x 4 threads, so a wave walks along one row.  The grid is sized by the largest frame; blocks beyond their own frame
//    return.  The colour map (64 KB for a 1080p frame's 136 x 240 map) stays in cache; the frame access decides the cost.
// Plain C++ loads and stores only.  Compiled with -ffp-contract=off like the other pre / post stages.
#include "common.h"
#include "draw_heat_host.h"

#define DH_BX 64
#define DH_BY 4
#define DH_BGR_PACKED 0
#define DH_BGR 1
#define DH_YUV 2
#define DH_RAGGED 6     // per row at most 3 pixels before the first aligned one and 3 after the last whole group

__global__ __launch_bounds__(DH_BX* DH_BY) void draw_heat_colormap_kernel(const float* __restrict__ maps, long long s0, long long s1, long long s2,
                                                                          long long s3, int C, int h, int w, long long total, DhStyle st,
                                                                          uint32_t* __restrict__ cm)
{
    const long long i = (long long)blockIdx.x * (DH_BX * DH_BY) + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % w);
    const long long r = i / w;
    const int y = (int)(r % h);
    const long long n = r / h;
    cm[i] = dh_cell(maps + n * s0 + y * s2 + x * s3, s1, C, st);
}

template <int MODE>
__global__ __launch_bounds__(DH_BX* DH_BY) void draw_heat_blend_kernel(const typename DrDesc<MODE == DH_YUV>::type* __restrict__ table,
                                                                       const uint32_t* __restrict__ cm, int h, int w, int opacity, int matrix)
{
    const typename DrDesc<MODE == DH_YUV>::type& d = table[blockIdx.z];
    const int H = d.H, W = d.W;
    const uint32_t* fcm = cm + (size_t)blockIdx.z * h * w;
    const int ux = blockIdx.x * DH_BX + threadIdx.x, uy = blockIdx.y * DH_BY + threadIdx.y;
    if constexpr (MODE == DH_YUV) {
        const int px = 2 * ux, py = 2 * uy;
        if (px >= W || py >= H) return;
        int luma[4], uv[2];
        dh_block_yuv(fcm, h, w, d.mi, px, py, H, W, matrix, luma, uv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = px + (q & 1), y = py + (q >> 1);
            if (x >= W || y >= H) continue;
            unsigned char* p = d.y_base + (long long)y * d.y_row + (long long)x * d.y_pix;
            *p = (unsigned char)do_blend(*p, luma[q], opacity);
        }
        const long long o = (long long)uy * d.c_row + (long long)ux * d.c_pix;
        d.u_base[o] = (unsigned char)do_blend(d.u_base[o], uv[0], opacity);
        d.v_base[o] = (unsigned char)do_blend(d.v_base[o], uv[1], opacity);
    } else {
        const int y = uy;
        if (y >= H) return;
        int x = ux;
        if constexpr (MODE == DH_BGR_PACKED) {
            // the row's colour bytes are [row, row + 3 W): pixel x starts at row + 3 x, which is 4-byte aligned iff x = row (mod 4)
            unsigned char* row = d.base + (long long)y * d.row_stride;
            const int lead = (int)((uintptr_t)row & 3);
            const int head = lead < W ? lead : W;
            const int groups = (W - head) >> 2, tail = W - head - 4 * groups;
            if (ux < groups) {
                const int x0 = head + 4 * ux;
                uint32_t* p = (uint32_t*)(row + 3ll * x0);
                const uint32_t in[3] = {p[0], p[1], p[2]};
                uint32_t out[3] = {0u, 0u, 0u};
                const bool rgb = d.ch_off[0] != 0;             // the byte order of a pixel: (B, G, R), or (R, G, B)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int c[3];
                    dh_sample(fcm, h, w, d.mi, x0 + q, y, c);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int i = 3 * q + j, s = 8 * (i & 3);
                        const int old = (int)((in[i >> 2] >> s) & 255u);
                        out[i >> 2] |= (uint32_t)do_blend(old, rgb ? c[2 - j] : c[j], opacity) << s;
                    }
                }
                p[0] = out[0];
                p[1] = out[1];
                p[2] = out[2];
                return;
            }
            const int e = ux - groups;                         // the ragged pixels of the row, one per thread
            if (e >= head + tail) return;
            x = e < head ? e : 4 * groups + e;
        } else {
            if (x >= W) return;
        }
        int c[3];
        dh_sample(fcm, h, w, d.mi, x, y, c);
        unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) p[d.ch_off[k]] = (unsigned char)do_blend(p[d.ch_off[k]], c[k], opacity);
    }
}

extern "C" int cp_sizeof_draw_heat_style(void) { return (int)sizeof(DhStyle); }
extern "C" size_t cp_draw_heat_scratch_bytes(int N, int h, int w) { return dh_scratch_bytes(N, h, w); }

// bgr HOST [n, 3] bytes (B, G, R) -> yuv HOST [n, 3] bytes (Y, U, V); matrix 0: BT.601, 1: BT.709
extern "C" int cp_bgr_to_yuv_host(const unsigned char* bgr, long long n, int matrix, unsigned char* yuv)
{
    CP_CHECK_ARG(n >= 0 && (n == 0 || (bgr && yuv)), "bgr_to_yuv_host: null pointer or negative count");
    CP_CHECK_ARG(matrix == 0 || matrix == 1, "bgr_to_yuv_host: matrix id %d is neither 0 (bt601) nor 1 (bt709)", matrix);
    for (long long i = 0; i < n; ++i) {
        int t[3];
        dh_bgr_to_yuv(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], matrix, t);
        for (int k = 0; k < 3; ++k) yuv[3 * i + k] = (unsigned char)t[k];
    }
    return 0;
}

#define DH_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

// table_host, maps, style HOST; the descriptors hold host addresses and, in `mi`, the frame -> map matrix
extern "C" int cp_draw_heat_frames_host(const void* table_host, int N, const float* maps, long long s0, long long s1, long long s2, long long s3,
                                        int C, int h, int w, const void* style)
{
    const long long stride[4] = {s0, s1, s2, s3};
    DH_FORWARD(dh_draw_frames_host<false>((const DrFrameDesc*)table_host, N, maps, stride, C, h, w, (const DhStyle*)style, 0, err, errn));
    return 0;
}

extern "C" int cp_draw_heat_yuv_frames_host(const void* table_host, int N, const float* maps, long long s0, long long s1, long long s2,
                                            long long s3, int C, int h, int w, const void* style, int matrix)
{
    const long long stride[4] = {s0, s1, s2, s3};
    DH_FORWARD(dh_draw_frames_host<true>((const DrYuvFrameDesc*)table_host, N, maps, stride, C, h, w, (const DhStyle*)style, matrix, err, errn));
    return 0;
}

// whether every frame of the table is packed: three colour bytes per pixel, back to back
static bool dh_all_packed(const DrFrameDesc* t, int N)
{
    for (int n = 0; n < N; ++n) {
        const DrFrameDesc& d = t[n];
        if (d.pix_stride != 3 || d.ch_off[1] != 1 || d.ch_off[0] + d.ch_off[2] != 2) return false;    // distinct offsets: (0,1,2) or (2,1,0)
    }
    return true;
}

template <bool YUV>
static int dh_launch(const char* who, const void* table, const void* table_host, int N, const float* maps, const long long* stride, int C, int h,
                     int w, const DhStyle* style, int matrix, void* scratch, size_t scratch_bytes, void* stream)
{
    typedef typename DrDesc<YUV>::type Desc;
    bool noop;
    DH_FORWARD(dh_check_call(who, N, stride, C, h, w, style, matrix, &noop, err, errn));
    if (noop) return 0;
    CP_CHECK_ARG(table && table_host && maps && scratch, "%s: null pointer", who);
    CP_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    CP_CHECK_ARG(scratch_bytes >= dh_scratch_bytes(N, h, w), "%s: scratch of %zu bytes, %zu needed (cp_draw_heat_scratch_bytes)", who,
                 scratch_bytes, dh_scratch_bytes(N, h, w));
    const Desc* th = (const Desc*)table_host;
    if constexpr (YUV) {
        DH_FORWARD(dr_check_yuv_frames(who, th, N, err, errn));
    } else {
        DH_FORWARD(dr_check_frames(who, th, N, err, errn));
    }
    DH_FORWARD(dh_check_matrices(who, th, N, err, errn));
    int maxH = 0, maxW = 0;
    for (int n = 0; n < N; ++n) {
        if (th[n].H > maxH) maxH = th[n].H;
        if (th[n].W > maxW) maxW = th[n].W;
    }
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)N * h * w;
    uint32_t* cm = (uint32_t*)scratch;
    const int threads = DH_BX * DH_BY;
    hipLaunchKernelGGL(draw_heat_colormap_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0, s, maps, stride[0],
                       stride[1], stride[2], stride[3], C, h, w, total, *style, cm);
    CP_CHECK_LAUNCH("draw_heat_colormap_kernel");
    const dim3 block(DH_BX, DH_BY);
    if constexpr (YUV) {
        const dim3 grid((unsigned)cp_cdiv(cp_cdiv(maxW, 2), DH_BX), (unsigned)cp_cdiv(cp_cdiv(maxH, 2), DH_BY), (unsigned)N);
        hipLaunchKernelGGL((draw_heat_blend_kernel<DH_YUV>), grid, block, 0, s, (const Desc*)table, (const uint32_t*)cm, h, w, style->opacity,
                           matrix);
        CP_CHECK_LAUNCH("draw_heat_blend_kernel<yuv>");
        cp_note_kernel("draw_heat_blend_kernel<yuv>");
    } else if (dh_all_packed(th, N)) {
        const dim3 grid((unsigned)cp_cdiv((maxW >> 2) + DH_RAGGED, DH_BX), (unsigned)cp_cdiv(maxH, DH_BY), (unsigned)N);
        hipLaunchKernelGGL((draw_heat_blend_kernel<DH_BGR_PACKED>), grid, block, 0, s, (const Desc*)table, (const uint32_t*)cm, h, w,
                           style->opacity, 0);
        CP_CHECK_LAUNCH("draw_heat_blend_kernel<bgr_packed>");
        cp_note_kernel("draw_heat_blend_kernel<bgr_packed>");
    } else {
        const dim3 grid((unsigned)cp_cdiv(maxW, DH_BX), (unsigned)cp_cdiv(maxH, DH_BY), (unsigned)N);
        hipLaunchKernelGGL((draw_heat_blend_kernel<DH_BGR>), grid, block, 0, s, (const Desc*)table, (const uint32_t*)cm, h, w, style->opacity, 0);
        CP_CHECK_LAUNCH("draw_heat_blend_kernel<bgr>");
        cp_note_kernel("draw_heat_blend_kernel<bgr>");
    }
    return 0;
}

// table DEVICE, table_host HOST (`mi`: the frame -> map matrix); maps DEVICE float32, element (n, c, i, j) at maps[n s0 + c s1 + i s2 + j s3];
// style HOST; scratch DEVICE, 16-byte aligned, at least cp_draw_heat_scratch_bytes(N, h, w) bytes
extern "C" int cp_draw_heat_frames_u8(const void* table, const void* table_host, int N, const float* maps, long long s0, long long s1,
                                      long long s2, long long s3, int C, int h, int w, const void* style, void* scratch, size_t scratch_bytes,
                                      void* stream)
{
    const long long stride[4] = {s0, s1, s2, s3};
    return dh_launch<false>("draw_heat_frames", table, table_host, N, maps, stride, C, h, w, (const DhStyle*)style, 0, scratch, scratch_bytes,
                            stream);
}

extern "C" int cp_draw_heat_yuv_frames_u8(const void* table, const void* table_host, int N, const float* maps, long long s0, long long s1,
                                          long long s2, long long s3, int C, int h, int w, const void* style, int matrix, void* scratch,
                                          size_t scratch_bytes, void* stream)
{
    const long long stride[4] = {s0, s1, s2, s3};
    return dh_launch<true>("draw_heat_yuv_frames", table, table_host, N, maps, stride, C, h, w, (const DhStyle*)style, matrix, scratch,
                           scratch_bytes, stream);
}
