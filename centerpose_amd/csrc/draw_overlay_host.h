// Host side of the overlay painters (draw_results with score labels and translucent primitives): the argument checks shared by the
// device launchers and the host painters, the scratch size, and the sequential host painters themselves (cp_draw_overlay_frames_host /
// cp_draw_overlay_yuv_frames_host, exported by draw_overlay.hip).  Plain C++ over draw_overlay_arith.h, no device code and no HIP
// header: tools/draw_overlay_host_fuzz.cpp compiles this file with the host compiler under AddressSanitizer / UBSan.  A failed check
// writes its message to `err` and returns 1.
//
// The host painters paint forward -- rows ascending, primitives in paint order, every covering primitive blended into what is there --
// where the device rasteriser first looks from the back for the topmost opaque cover and blends only what lies above it: two routes
// to the one picture draw_overlay_arith.h defines.
#pragma once
#include "draw_host.h"
#include "draw_overlay_arith.h"

// scratch of one call: the row headers and primitive records of draw_host.h, then one label record per row
inline size_t do_scratch_bytes(long long N, long long M)
{
    if (N <= 0 || M <= 0) return 0;
    return dr_scratch_bytes(N, M) + (size_t)N * (size_t)M * sizeof(DoLabel);
}

inline int do_check_overlay(const char* who, const DoOverlay* ov, char* err, size_t errn)
{
    DR_CHECK(ov, "%s: null overlay", who);
    for (int i = 0; i < 3; ++i)
        DR_CHECK(ov->opacity[i] >= 1 && ov->opacity[i] <= DO_OPAQUE, "%s: opacity %d (%s) outside 1..%d", who, ov->opacity[i],
                 i == 0 ? "box" : (i == 1 ? "limbs" : "joints"), DO_OPAQUE);
    DR_CHECK(ov->label_scale >= 0 && ov->label_scale <= DT_MAX_SCALE, "%s: label_scale %d outside 0..%d", who, ov->label_scale, DT_MAX_SCALE);
    DR_CHECK(ov->nprefix >= 0 && ov->nprefix <= DO_MAX_PREFIX, "%s: a label prefix of %d glyphs, 0..%d are drawn", who, ov->nprefix,
             DO_MAX_PREFIX);
    for (int i = 0; i < ov->nprefix; ++i)
        DR_CHECK(ov->prefix[i] < DT_GLYPHS, "%s: prefix glyph %d is index %d, the font has %d", who, i, (int)ov->prefix[i], DT_GLYPHS);
    return 0;
}

// row_ids and the id palette come together or not at all
inline int do_check_ids(const char* who, const int* row_ids, const DaIdPalette* idp, char* err, size_t errn)
{
    DR_CHECK((row_ids != nullptr) == (idp != nullptr), "%s: row_ids and the id palette are given together or not at all", who);
    if (idp) return dr_check_ids(who, row_ids, idp, err, errn);
    return 0;
}

// Primitive by primitive over the S x S blocks that meet its bounds (clipped to the H x W frame): pix(x, y) for every covered in-frame
// pixel, then blk(X, Y) once for a block with at least one.
template <int S, class Cover, class Pix, class Blk>
inline void do_paint_prim(int x0, int y0, int x1, int y1, int H, int W, Cover cover, Pix pix, Blk blk)
{
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > W - 1) x1 = W - 1;
    if (y1 > H - 1) y1 = H - 1;
    if (x0 > x1 || y0 > y1) return;
    for (int Y = y0 / S; Y <= y1 / S; ++Y)
        for (int X = x0 / S; X <= x1 / S; ++X) {
            bool any = false;
            for (int q = 0; q < S * S; ++q) {
                const int x = X * S + q % S, y = Y * S + q / S;
                if (x < W && y < H && cover(x, y)) {
                    pix(x, y);
                    any = true;
                }
            }
            if (any) blk(X, Y);
        }
}

// HOST painter over cp_frame_desc (YUV = false) or cp_yuv_frame_desc (true) descriptors with host addresses; row_ids / idp may both
// be null.  Colours are what the frames hold: (B, G, R) in channel order 0..2, or (Y, U, V).
template <bool YUV>
inline int do_draw_frames_host(const typename DrDesc<YUV>::type* table, int N, const float* rows, int M, float vis_thresh, const DaStyle* style,
                               const int* row_ids, const DaIdPalette* idp, const DoOverlay* ov, char* err, size_t errn)
{
    const char* who = YUV ? "draw_overlay_yuv_frames_host" : "draw_overlay_frames_host";
    constexpr int S = YUV ? 2 : 1;
    bool noop;
    if (int rc = dr_check_call(who, N, M, vis_thresh, style, &noop, err, errn)) return rc;
    if (int rc = do_check_overlay(who, ov, err, errn)) return rc;
    if (noop) return 0;
    DR_CHECK(table && rows, "%s: null pointer", who);
    if (int rc = do_check_ids(who, row_ids, idp, err, errn)) return rc;
    if constexpr (YUV) {
        if (int rc = dr_check_yuv_frames(who, table, N, err, errn)) return rc;
    } else {
        if (int rc = dr_check_frames(who, table, N, err, errn)) return rc;
    }
    const int T = style->box_thickness, RL = style->limb_radius, RJ = style->joint_radius, s = ov->label_scale;
    for (int n = 0; n < N; ++n) {
        const auto& d = table[n];
        for (int m = 0; m < M; ++m) {
            const float* row = rows + ((size_t)n * M + m) * DA_ROW;
            if (!da_live(row, vis_thresh)) continue;
            const int id = row_ids ? row_ids[(size_t)n * M + m] : -1;
            DaPrim prims[DA_PRIMS];
            DoLabel lb;
            uint64_t mask = 0;
            for (int l = 0; l < DA_PRIMS; ++l)
                if (da_reach(T, RL, RJ, l) >= 0 && da_build(row, l, &prims[l])) mask |= 1ull << l;
            if (do_build_label(row, *ov, &lb)) mask |= (1ull << DO_BAR) | (1ull << DO_TEXT);
            for (int l = 0; l < DO_PRIMS; ++l) {
                if (!((mask >> l) & 1)) continue;
                int x0, y0, x1, y1;
                if (l < DA_PRIMS)
                    da_bounds(prims[l], da_reach(T, RL, RJ, l), &x0, &y0, &x1, &y1);
                else
                    do_label_bounds(lb, s, &x0, &y0, &x1, &y1);
                int c[3];
                do_color(*style, *ov, idp, id, l, c);
                const int a = do_opacity(*ov, l);
                auto cover = [&](int x, int y) { return do_covers(prims, lb, l, T, RL, RJ, s, x, y); };
                if constexpr (YUV) {
                    do_paint_prim<S>(
                        x0, y0, x1, y1, d.H, d.W, cover,
                        [&](int x, int y) {
                            unsigned char* p = d.y_base + (long long)y * d.y_row + (long long)x * d.y_pix;
                            *p = (unsigned char)do_blend(*p, c[0], a);
                        },
                        [&](int X, int Y) {
                            const long long o = (long long)Y * d.c_row + (long long)X * d.c_pix;
                            d.u_base[o] = (unsigned char)do_blend(d.u_base[o], c[1], a);
                            d.v_base[o] = (unsigned char)do_blend(d.v_base[o], c[2], a);
                        });
                } else {
                    do_paint_prim<S>(
                        x0, y0, x1, y1, d.H, d.W, cover,
                        [&](int x, int y) {
                            unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
                            for (int k = 0; k < 3; ++k) p[d.ch_off[k]] = (unsigned char)do_blend(p[d.ch_off[k]], c[k], a);
                        },
                        [](int, int) {});
                }
            }
        }
    }
    return 0;
}
