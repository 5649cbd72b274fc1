// Host side of draw_tracks: the argument checks shared by the device launchers and the host painters, and the sequential host painters
// themselves (cp_draw_tracks_frames_host / cp_draw_tracks_yuv_frames_host, exported by draw_tracks.hip).  Plain C++ over
// draw_text_arith.h and the frame checks of draw_host.h, no device code and no HIP header: tools/draw_tracks_host_fuzz.cpp compiles this
// file with the host compiler under AddressSanitizer / UBSan.  A failed check writes its message to `err` and returns 1.
//
// The host painters paint forward -- items ascending, box then bar then text, a later store over an earlier one -- where the device
// rasteriser looks for the last covering primitive from the back: two routes to the one picture draw_text_arith.h defines.
#pragma once
#include "draw_host.h"
#include "draw_text_arith.h"

// what does not depend on the frames: N, Kmax, T, s.  *noop: nothing to paint (N or Kmax is 0), nothing else is looked at.
inline int dk_check_call(const char* who, int N, int Kmax, int T, int s, bool* noop, char* err, size_t errn)
{
    *noop = false;
    DR_CHECK(N >= 0 && N <= 65535, "%s: 0 to 65535 frames per call (got %d)", who, N);
    DR_CHECK(Kmax >= 0, "%s: negative item count %d", who, Kmax);
    DR_CHECK((long long)N * Kmax <= DT_MAX_ITEMS, "%s: %d x %d items are too many for one call (at most %d)", who, N, Kmax, DT_MAX_ITEMS);
    DR_CHECK(T >= 0 && T <= DA_MAX_REACH, "%s: box_thickness %d outside 0..%d", who, T, DA_MAX_REACH);
    DR_CHECK(s >= 0 && s <= DT_MAX_SCALE, "%s: font_scale %d outside 0..%d", who, s, DT_MAX_SCALE);
    *noop = N == 0 || Kmax == 0;
    return 0;
}

// the HOST copy of the item table: counts, label lengths, glyph indices, corners.  *total: the items of the call.
inline int dk_check_items(const char* who, const DtItem* items, const int* counts, int N, int Kmax, long long* total, char* err, size_t errn)
{
    *total = 0;
    for (int n = 0; n < N; ++n) {
        DR_CHECK(counts[n] >= 0 && counts[n] <= Kmax, "%s: frame %d: %d items outside 0..Kmax = %d", who, n, counts[n], Kmax);
        *total += counts[n];
        for (int k = 0; k < counts[n]; ++k) {
            const DtItem& it = items[(size_t)n * Kmax + k];
            DR_CHECK(it.nchars >= 0 && it.nchars <= DT_MAX_CHARS, "%s: frame %d item %d: %d characters outside 0..%d", who, n, k, it.nchars,
                     DT_MAX_CHARS);
            for (int c = 0; c < it.nchars; ++c)
                DR_CHECK(it.glyph[c] < DT_GLYPHS, "%s: frame %d item %d: glyph index %d outside the font (0..%d)", who, n, k, it.glyph[c],
                         DT_GLYPHS - 1);
            DR_CHECK(it.x0 >= -DA_MAX_SIDE && it.y0 >= -DA_MAX_SIDE && it.x1 < DA_MAX_SIDE && it.y1 < DA_MAX_SIDE && it.x0 <= it.x1 &&
                         it.y0 <= it.y1,
                     "%s: frame %d item %d: corners (%d, %d) (%d, %d) are not sorted inside [-16384, 16383]", who, n, k, it.x0, it.y0, it.x1,
                     it.y1);
        }
    }
    return 0;
}

// The pixels of one item in paint order: put(x, y, l) for every pixel of the H x W frame that primitive l covers.
template <class Put>
inline void dk_paint_item(const DtItem& it, int T, int s, int H, int W, Put put)
{
    int x0, y0, x1, y1;
    dt_bounds(it, s, &x0, &y0, &x1, &y1);
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > W - 1) x1 = W - 1;
    if (y1 > H - 1) y1 = H - 1;
    for (int l = 0; l < DT_PRIMS; ++l)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x)
                if (dt_covers(it, l, T, s, x, y)) put(x, y, l);
}

// HOST painter over cp_frame_desc descriptors with host addresses
inline int dk_draw_frames_host(const DrFrameDesc* table, int N, const DtItem* items, const int* counts, int Kmax, int T, int s, char* err,
                               size_t errn)
{
    const char* who = "draw_tracks_frames_host";
    bool noop;
    long long total;
    if (int rc = dk_check_call(who, N, Kmax, T, s, &noop, err, errn)) return rc;
    if (noop) return 0;
    DR_CHECK(table && items && counts, "%s: null pointer", who);
    if (int rc = dk_check_items(who, items, counts, N, Kmax, &total, err, errn)) return rc;
    if (int rc = dr_check_frames(who, table, N, err, errn)) return rc;
    for (int n = 0; n < N; ++n) {
        const DrFrameDesc& d = table[n];
        for (int k = 0; k < counts[n]; ++k) {
            const DtItem& it = items[(size_t)n * Kmax + k];
            dk_paint_item(it, T, s, d.H, d.W, [&](int x, int y, int l) {
                unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
                const unsigned char* c = l == 2 ? it.text_color : it.color;
                for (int j = 0; j < 3; ++j) p[d.ch_off[j]] = c[j];
            });
        }
    }
    return 0;
}

// HOST painter over cp_yuv_frame_desc descriptors with host addresses; item colours are (Y, U, V).  Every covered pixel stores its
// luma and the chroma sample of its 2x2 block, so the sample ends with the colour of the last primitive that covers any of the four.
inline int dk_draw_yuv_frames_host(const DrYuvFrameDesc* table, int N, const DtItem* items, const int* counts, int Kmax, int T, int s,
                                   char* err, size_t errn)
{
    const char* who = "draw_tracks_yuv_frames_host";
    bool noop;
    long long total;
    if (int rc = dk_check_call(who, N, Kmax, T, s, &noop, err, errn)) return rc;
    if (noop) return 0;
    DR_CHECK(table && items && counts, "%s: null pointer", who);
    if (int rc = dk_check_items(who, items, counts, N, Kmax, &total, err, errn)) return rc;
    if (int rc = dr_check_yuv_frames(who, table, N, err, errn)) return rc;
    for (int n = 0; n < N; ++n) {
        const DrYuvFrameDesc& d = table[n];
        for (int k = 0; k < counts[n]; ++k) {
            const DtItem& it = items[(size_t)n * Kmax + k];
            dk_paint_item(it, T, s, d.H, d.W, [&](int x, int y, int l) {
                const unsigned char* c = l == 2 ? it.text_color : it.color;
                const long long o = (long long)(y >> 1) * d.c_row + (long long)(x >> 1) * d.c_pix;
                d.y_base[(long long)y * d.y_row + (long long)x * d.y_pix] = c[0];
                d.u_base[o] = c[1];
                d.v_base[o] = c[2];
            });
        }
    }
    return 0;
}
