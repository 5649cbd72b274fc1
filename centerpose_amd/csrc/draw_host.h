// Host side of draw_results: the descriptor mirrors, the argument checks shared by the device launchers and the host painters, and the
// sequential host painters themselves (cp_draw_rows_frames_host / cp_draw_rows_yuv_frames_host, exported by draw_results.hip).  Plain
// C++ over draw_arith.h, no device code and no HIP header: tools/draw_host_fuzz.cpp compiles this file with the host compiler under
// AddressSanitizer / UBSan.  A failed check writes its message to `err` and returns 1.
//
// The host painters paint forward -- rows ascending, primitives in paint order, a later store over an earlier one -- where the
// device rasteriser looks for the last covering primitive from the back: two routes to the one picture draw_arith.h defines.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include "draw_arith.h"

// mirror of cp_frame_desc (include/centerpose_hip.h); drawing reads base, the strides, ch_off, H and W
struct DrFrameDesc {
    unsigned char* base;
    long long row_stride, pix_stride;
    long long ch_off[3];
    long long mid_off;
    int H, W, NH, NW;
    double mi[6];
    int slot, pad;
};
static_assert(sizeof(DrFrameDesc) == 128, "cp_frame_desc is 128 bytes");

// mirror of cp_yuv_frame_desc; drawing reads the bases, the strides, H and W
struct DrYuvFrameDesc {
    unsigned char* y_base;
    long long y_row, y_pix;
    unsigned char* u_base;
    unsigned char* v_base;
    long long c_row, c_pix;
    long long mid_off;
    int H, W, NH, NW;
    double mi[6];
    int slot, pad;
};
static_assert(sizeof(DrYuvFrameDesc) == 136, "cp_yuv_frame_desc is 136 bytes");

// the descriptor type of a painter instantiated for BGR / RGB frames (false) or YUV frames (true)
template <bool YUV>
struct DrDesc { typedef DrFrameDesc type; };
template <>
struct DrDesc<true> { typedef DrYuvFrameDesc type; };

// scratch of one call: per row a header (bounding box, mask of existing primitives), then the primitive records of all rows
struct DrRowHeader { int x0, y0, x1, y1; unsigned long long mask; unsigned long long pad; };
static_assert(sizeof(DrRowHeader) == 32, "row header is 32 bytes");
#define DR_MAX_ROWS (1ll << 28)
#define DR_MAX_M (1 << 24)      // a paint index, row * 36 + primitive, fits an int

inline size_t dr_scratch_bytes(long long N, long long M)
{
    if (N <= 0 || M <= 0) return 0;
    return (size_t)N * (size_t)M * (sizeof(DrRowHeader) + DA_PRIMS * sizeof(DaPrim));
}

#define DR_CHECK(cond, ...)                      \
    do {                                         \
        if (!(cond)) {                           \
            snprintf(err, errn, __VA_ARGS__);    \
            return 1;                            \
        }                                        \
    } while (0)

// what does not depend on the frames: N, M, vis_thresh, the style.  *noop: nothing to paint (N or M is 0), nothing else is looked at.
inline int dr_check_call(const char* who, int N, int M, float vis_thresh, const DaStyle* style, bool* noop, char* err, size_t errn)
{
    *noop = false;
    DR_CHECK(N >= 0 && N <= 65535, "%s: 0 to 65535 frames per call (got %d)", who, N);
    DR_CHECK(M >= 0, "%s: negative row count %d", who, M);
    DR_CHECK(M <= DR_MAX_M, "%s: at most %d rows per frame (got %d)", who, DR_MAX_M, M);
    DR_CHECK((long long)N * M <= DR_MAX_ROWS, "%s: %d x %d rows are too many for one call", who, N, M);
    DR_CHECK(da_finite(vis_thresh), "%s: vis_thresh is not finite", who);
    DR_CHECK(style, "%s: null style", who);
    DR_CHECK(style->box_thickness >= 0 && style->box_thickness <= DA_MAX_REACH, "%s: box_thickness %d outside 0..%d", who,
             style->box_thickness, DA_MAX_REACH);
    DR_CHECK(style->limb_radius == -1 || (style->limb_radius >= 1 && style->limb_radius <= DA_MAX_REACH),
             "%s: limb_radius %d is neither -1 nor in 1..%d", who, style->limb_radius, DA_MAX_REACH);
    DR_CHECK(style->joint_radius >= -1 && style->joint_radius <= DA_MAX_REACH, "%s: joint_radius %d outside -1..%d", who,
             style->joint_radius, DA_MAX_REACH);
    *noop = N == 0 || M == 0;
    return 0;
}

// the two arguments of the identity-coloured forms come together or not at all
inline int dr_check_ids(const char* who, const int* row_ids, const DaIdPalette* idp, char* err, size_t errn)
{
    DR_CHECK(row_ids && idp, "%s: null row_ids or id palette", who);
    DR_CHECK(idp->count >= 1 && idp->count <= DA_MAX_ID_COLORS, "%s: %d id colours outside 1..%d", who, idp->count, DA_MAX_ID_COLORS);
    return 0;
}

inline int dr_check_frames(const char* who, const DrFrameDesc* t, int N, char* err, size_t errn)
{
    for (int n = 0; n < N; ++n) {
        const DrFrameDesc& d = t[n];
        DR_CHECK(d.base, "%s: frame %d: null base address", who, n);
        DR_CHECK(d.H >= 1 && d.H <= DA_MAX_SIDE && d.W >= 1 && d.W <= DA_MAX_SIDE, "%s: frame %d: bad size %d x %d (1..%d)", who, n, d.H,
                 d.W, DA_MAX_SIDE);
        DR_CHECK(d.row_stride >= 0 && d.pix_stride >= 0 && d.ch_off[0] >= 0 && d.ch_off[1] >= 0 && d.ch_off[2] >= 0,
                 "%s: frame %d: negative stride or channel offset", who, n);
        DR_CHECK((d.H == 1 || d.row_stride > 0) && (d.W == 1 || d.pix_stride > 0), "%s: frame %d: a stride of 0 cannot be written", who, n);
        DR_CHECK(d.ch_off[0] != d.ch_off[1] && d.ch_off[1] != d.ch_off[2] && d.ch_off[0] != d.ch_off[2],
                 "%s: frame %d: two channels at one offset cannot be written", who, n);
        long long ch_max = d.ch_off[0];
        if (d.ch_off[1] > ch_max) ch_max = d.ch_off[1];
        if (d.ch_off[2] > ch_max) ch_max = d.ch_off[2];
        const __int128 last = (__int128)(d.H - 1) * d.row_stride + (__int128)(d.W - 1) * d.pix_stride + ch_max;
        DR_CHECK(last < ((__int128)1 << 62), "%s: frame %d: strides address more than 2^62 bytes", who, n);
    }
    return 0;
}

inline int dr_check_yuv_frames(const char* who, const DrYuvFrameDesc* t, int N, char* err, size_t errn)
{
    for (int n = 0; n < N; ++n) {
        const DrYuvFrameDesc& d = t[n];
        DR_CHECK(d.pad == 0, "%s: frame %d: format word pad = %d: only 8-bit 4:2:0 frames (pad 0) can be drawn on", who, n, d.pad);
        DR_CHECK(d.y_base && d.u_base && d.v_base, "%s: frame %d: null base address (y %p, u %p, v %p)", who, n, (const void*)d.y_base,
                 (const void*)d.u_base, (const void*)d.v_base);
        DR_CHECK(d.H >= 1 && d.H <= DA_MAX_SIDE && d.W >= 1 && d.W <= DA_MAX_SIDE, "%s: frame %d: bad size %d x %d (1..%d)", who, n, d.H,
                 d.W, DA_MAX_SIDE);
        DR_CHECK(d.y_row >= 0 && d.y_pix >= 0 && d.c_row >= 0 && d.c_pix >= 0, "%s: frame %d: negative stride", who, n);
        DR_CHECK((d.H == 1 || d.y_row > 0) && (d.W == 1 || d.y_pix > 0) && (d.H <= 2 || d.c_row > 0) && (d.W <= 2 || d.c_pix > 0),
                 "%s: frame %d: a stride of 0 cannot be written", who, n);
        DR_CHECK(d.u_base != d.v_base, "%s: frame %d: U and V at one address cannot be written", who, n);
        const __int128 y_last = (__int128)(d.H - 1) * d.y_row + (__int128)(d.W - 1) * d.y_pix;
        const __int128 c_last = (__int128)((d.H - 1) >> 1) * d.c_row + (__int128)((d.W - 1) >> 1) * d.c_pix;
        DR_CHECK(y_last < ((__int128)1 << 62) && c_last < ((__int128)1 << 62), "%s: frame %d: strides address more than 2^62 bytes", who, n);
    }
    return 0;
}

// The pixels of one live row in paint order: put(x, y, l) for every pixel of the H x W frame that primitive l covers.
template <class Put>
inline void dr_paint_row(const float* row, const DaStyle& s, int H, int W, Put put)
{
    for (int l = 0; l < DA_PRIMS; ++l) {
        const int reach = da_reach(s.box_thickness, s.limb_radius, s.joint_radius, l);
        DaPrim p;
        if (reach < 0 || !da_build(row, l, &p)) continue;
        int x0, y0, x1, y1;
        da_bounds(p, reach, &x0, &y0, &x1, &y1);
        if (x0 < 0) x0 = 0;
        if (y0 < 0) y0 = 0;
        if (x1 > W - 1) x1 = W - 1;
        if (y1 > H - 1) y1 = H - 1;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x)
                if (da_covers(p, l, s.box_thickness, s.limb_radius, s.joint_radius, x, y)) put(x, y, l);
    }
}

// HOST painter over cp_frame_desc descriptors with host addresses
// (ids: with row_ids int [N, M] and an id palette, a row whose id is >= 0 stores colors[id % count] for all of its primitives)
inline int dr_draw_frames_host(const DrFrameDesc* table, int N, const float* rows, int M, float vis_thresh, const DaStyle* style, char* err,
                               size_t errn, bool ids = false, const int* row_ids = nullptr, const DaIdPalette* idp = nullptr)
{
    const char* who = ids ? "draw_rows_ids_frames_host" : "draw_rows_frames_host";
    bool noop;
    if (int rc = dr_check_call(who, N, M, vis_thresh, style, &noop, err, errn)) return rc;
    if (noop) return 0;
    DR_CHECK(table && rows, "%s: null pointer", who);
    if (ids)
        if (int rc = dr_check_ids(who, row_ids, idp, err, errn)) return rc;
    if (int rc = dr_check_frames(who, table, N, err, errn)) return rc;
    for (int n = 0; n < N; ++n) {
        const DrFrameDesc& d = table[n];
        for (int m = 0; m < M; ++m) {
            const float* row = rows + ((size_t)n * M + m) * DA_ROW;
            if (!da_live(row, vis_thresh)) continue;
            const int id = ids ? row_ids[(size_t)n * M + m] : -1;
            dr_paint_row(row, *style, d.H, d.W, [&](int x, int y, int l) {
                unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
                const unsigned char* c = da_color(*style, ids ? idp : nullptr, id, l);
                for (int k = 0; k < 3; ++k) p[d.ch_off[k]] = c[k];
            });
        }
    }
    return 0;
}

// HOST painter over cp_yuv_frame_desc descriptors with host addresses; palette entries are (Y, U, V).  Every covered pixel stores its
// luma and the chroma sample of its 2x2 block, so the sample ends with the colour of the last primitive that covers any of the four.
inline int dr_draw_yuv_frames_host(const DrYuvFrameDesc* table, int N, const float* rows, int M, float vis_thresh, const DaStyle* style,
                                   char* err, size_t errn, bool ids = false, const int* row_ids = nullptr, const DaIdPalette* idp = nullptr)
{
    const char* who = ids ? "draw_rows_ids_yuv_frames_host" : "draw_rows_yuv_frames_host";
    bool noop;
    if (int rc = dr_check_call(who, N, M, vis_thresh, style, &noop, err, errn)) return rc;
    if (noop) return 0;
    DR_CHECK(table && rows, "%s: null pointer", who);
    if (ids)
        if (int rc = dr_check_ids(who, row_ids, idp, err, errn)) return rc;
    if (int rc = dr_check_yuv_frames(who, table, N, err, errn)) return rc;
    for (int n = 0; n < N; ++n) {
        const DrYuvFrameDesc& d = table[n];
        for (int m = 0; m < M; ++m) {
            const float* row = rows + ((size_t)n * M + m) * DA_ROW;
            if (!da_live(row, vis_thresh)) continue;
            const int id = ids ? row_ids[(size_t)n * M + m] : -1;
            dr_paint_row(row, *style, d.H, d.W, [&](int x, int y, int l) {
                const long long c = (long long)(y >> 1) * d.c_row + (long long)(x >> 1) * d.c_pix;
                const unsigned char* col = da_color(*style, ids ? idp : nullptr, id, l);
                d.y_base[(long long)y * d.y_row + (long long)x * d.y_pix] = col[0];
                d.u_base[c] = col[1];
                d.v_base[c] = col[2];
            });
        }
    }
    return 0;
}
