// The drawing rule of the overlay painters, once, for the host and the device: draw_results with a score label on every box and with
// translucent primitives.  draw_overlay.hip compiles these statements into its two kernels, draw_overlay_host.h into the sequential
// host painters (what a test pins).  Integer-only after the coordinate conversion of draw_arith.h.
//
// The 38 primitives of a row in paint order: the 36 of draw_arith.h (0 the box, 1..18 the limbs, 19..35 the joints), then 36 the label
// bar and 37 the label text.  The paint index is row * 38 + primitive, rows ascending.
//
// Blend.  Primitive l has an opacity a in 1..256: the style's box opacity for 0, limb opacity for 1..18, joint opacity for 19..35, and
// always 256 for the bar and the text.  A covered channel byte p becomes (p * (256 - a) + c * a + 128) >> 8, once per covering
// primitive, in paint order.  a = 256 gives c exactly; c = p gives p for every a.  On YUV frames luma is blended per covered pixel and
// chroma sample (i, j) once per primitive that covers at least one in-frame pixel of its 2 x 2 block, with that primitive's (U, V).
//
// Label.  A live row has one when label_scale s is in 1..8 and its four box coordinates are alive (box_thickness plays no part).  With
// (x0, y0) the sorted corner of the box primitive, n characters, tw = 6 s n - s and th = 7 s:
//   36 the bar  : the closed rectangle [x0, x0 + tw + 3] x [y0 - th - 5, y0 - 1]: the bar of draw_text_arith.h, sitting on the box
//   37 the text : the glyph rule of draw_text_arith.h with dx = x - (x0 + 2), dy = y - (y0 - th - 3)
// The bar stores what the row's box stores (palette[0], or the identity colour), the text the overlay's text colour.
//
// Label text: the prefix (0..9 glyph indices) and the score to one decimal, by an integer rule on the float's bits.  With |score| =
// m 2^e exactly, t = min(round_half_even(10 m 2^e), 9999); the text is ['-' if the sign bit is set] str(t / 10) '.' str(t % 10).
// +-inf gives 999.9; NaN never arrives (da_live is false for it).  At most 9 + 1 + 3 + 1 + 1 = 15 characters.
#pragma once
#include "draw_text_arith.h"

#define DO_PRIMS 38
#define DO_BAR 36
#define DO_TEXT 37
#define DO_MAX_PREFIX 9
#define DO_OPAQUE 256
#define DO_GLYPH_MINUS 38
#define DO_GLYPH_POINT 39

// mirror of cp_draw_overlay (include/centerpose_hip.h)
struct DoOverlay {
    int opacity[3];                     // box, limbs, joints: 1..256
    int label_scale;                    // 0: no labels, 1..8: pixels per font cell
    int nprefix;                        // 0..9
    unsigned char prefix[12];           // glyph indices, the first nprefix are read
    unsigned char text_color[4];        // bytes 0..2: what the label text stores; byte 3 is not used
};
static_assert(sizeof(DoOverlay) == 36, "cp_draw_overlay is 36 bytes");

// the label of one row as the build step leaves it: (x0, y0) is the top-left corner of the BAR; nchars = 0: the row has no label
struct DoLabel {
    int x0, y0;
    int nchars;
    int pad;
    unsigned char glyph[DT_MAX_CHARS];
};
static_assert(sizeof(DoLabel) == 32, "label record is 32 bytes");

DA_HD int do_opacity(const DoOverlay& ov, int l)
{
    if (l == 0) return ov.opacity[0];
    if (l <= DA_LIMBS) return ov.opacity[1];
    return l < DA_PRIMS ? ov.opacity[2] : DO_OPAQUE;
}

// the primitives of a row that store their colour outright, as a mask over the 38
DA_HD uint64_t do_opaque_mask(const DoOverlay& ov)
{
    uint64_t m = (1ull << DO_BAR) | (1ull << DO_TEXT);
    if (ov.opacity[0] == DO_OPAQUE) m |= 1ull;
    if (ov.opacity[1] == DO_OPAQUE) m |= ((1ull << DA_LIMBS) - 1) << 1;
    if (ov.opacity[2] == DO_OPAQUE) m |= ((1ull << DA_JOINTS) - 1) << (1 + DA_LIMBS);
    return m;
}

DA_HD int do_blend(int p, int c, int a) { return (p * (DO_OPAQUE - a) + c * a + 128) >> 8; }

// what primitive l of a row stores, by value: bytes 0..2 into c
DA_HD void do_color(const DaStyle& st, const DoOverlay& ov, const DaIdPalette* idp, int id, int l, int* c)
{
    if (l == DO_TEXT) {
        c[0] = ov.text_color[0]; c[1] = ov.text_color[1]; c[2] = ov.text_color[2];
    } else if (idp && id >= 0) {
        const int i = id % idp->count;
        c[0] = idp->colors[i][0]; c[1] = idp->colors[i][1]; c[2] = idp->colors[i][2];
    } else {
        const int e = l == DO_BAR ? 0 : l;
        c[0] = st.palette[e][0]; c[1] = st.palette[e][1]; c[2] = st.palette[e][2];
    }
}

// The score to one decimal as glyph indices -> the number of glyphs written (3..6), -1 for NaN (nothing is written).
DA_HD int do_score_glyphs(float score, unsigned char* g)
{
    union { float f; uint32_t u; } c;
    c.f = score;
    const uint32_t ex = (c.u >> 23) & 0xffu, man = c.u & 0x7fffffu;
    if (ex == 0xffu && man != 0) return -1;
    uint32_t t;
    if (ex == 0xffu || ex >= 150u) {
        t = 9999;                                              // inf, or at least 2^23
    } else if (ex == 0 || 150u - ex >= 40u) {
        t = 0;                                                 // 10 m < 2^28: below 2^-12
    } else {
        const unsigned k = 150u - ex;                          // |score| = m / 2^k, 1 <= k < 40
        const uint64_t P = 10ull * (man | 0x800000u), half = 1ull << (k - 1), rem = P & ((1ull << k) - 1);
        uint64_t q = P >> k;
        if (rem > half || (rem == half && (q & 1))) ++q;       // to nearest, ties to even
        t = q > 9999 ? 9999u : (uint32_t)q;
    }
    int n = 0;
    if (c.u >> 31) g[n++] = DO_GLYPH_MINUS;
    const uint32_t whole = t / 10;
    if (whole >= 100) g[n++] = (unsigned char)(whole / 100);
    if (whole >= 10) g[n++] = (unsigned char)(whole / 10 % 10);
    g[n++] = (unsigned char)(whole % 10);
    g[n++] = DO_GLYPH_POINT;
    g[n++] = (unsigned char)(t % 10);
    return n;
}

DA_HD int do_text_w(int nchars, int s) { return 6 * s * nchars - s; }
DA_HD int do_text_h(int s) { return 7 * s; }

// The label of a live row: whether it has one, and its record.  Without one the record says so (nchars = 0).
DA_HD bool do_build_label(const float* row, const DoOverlay& ov, DoLabel* lb)
{
    lb->x0 = 0; lb->y0 = 0; lb->nchars = 0; lb->pad = 0;
    for (int i = 0; i < DT_MAX_CHARS; ++i) lb->glyph[i] = 0;
    DaPrim box;
    if (ov.label_scale <= 0 || !da_build(row, 0, &box)) return false;
    unsigned char sg[6];
    const int ns = do_score_glyphs(row[4], sg);
    if (ns < 0) return false;                                  // NaN: not live, never here
    int n = 0;
    for (int i = 0; i < ov.nprefix && i < DO_MAX_PREFIX; ++i) lb->glyph[n++] = ov.prefix[i];
    for (int i = 0; i < ns; ++i) lb->glyph[n++] = sg[i];
    lb->nchars = n;
    lb->x0 = box.x0;
    lb->y0 = box.y0 - do_text_h(ov.label_scale) - 5;
    return true;
}

// the bounding box of a label: its bar
DA_HD void do_label_bounds(const DoLabel& lb, int s, int* x0, int* y0, int* x1, int* y1)
{
    *x0 = lb.x0; *y0 = lb.y0;
    *x1 = lb.x0 + do_text_w(lb.nchars, s) + 3; *y1 = lb.y0 + do_text_h(s) + 4;
}

// whether primitive l (DO_BAR or DO_TEXT) of a label (nchars > 0, s >= 1) covers pixel (x, y)
DA_HD bool do_label_covers(const DoLabel& lb, int l, int s, int x, int y)
{
    const int tw = do_text_w(lb.nchars, s), th = do_text_h(s);
    if (l == DO_BAR) return x >= lb.x0 && x <= lb.x0 + tw + 3 && y >= lb.y0 && y <= lb.y0 + th + 4;
    const int dx = x - (lb.x0 + 2), dy = y - (lb.y0 + 2);
    if (dx < 0 || dx >= tw || dy < 0 || dy >= th) return false;
    const int cell = dx / (6 * s), u = (dx - cell * 6 * s) / s;
    if (u >= 5 || cell >= DT_MAX_CHARS) return false;           // cell < nchars <= 15
    return (dt_font_row(lb.glyph[cell], dy / s) >> (4 - u)) & 1u;
}

// whether primitive l (0..37) of a row covers (x, y); the row has it (its bit in the row's mask is set)
DA_HD bool do_covers(const DaPrim* prims, const DoLabel& lb, int l, int box_thickness, int limb_radius, int joint_radius, int s, int x, int y)
{
    if (l >= DA_PRIMS) return do_label_covers(lb, l, s, x, y);
    return da_covers(prims[l], l, box_thickness, limb_radius, joint_radius, x, y);
}

// the last primitive of one row, among those in `mask` (38 bits), that covers (x, y), scanning from the back; -1: none
DA_HD int do_row_winner(const DaPrim* prims, const DoLabel& lb, uint64_t mask, int box_thickness, int limb_radius, int joint_radius, int s, int x,
                        int y)
{
    if (((mask >> DO_TEXT) & 1) && do_label_covers(lb, DO_TEXT, s, x, y)) return DO_TEXT;
    if (((mask >> DO_BAR) & 1) && do_label_covers(lb, DO_BAR, s, x, y)) return DO_BAR;
    return da_row_winner(prims, mask & ((1ull << DA_PRIMS) - 1), box_thickness, limb_radius, joint_radius, x, y);
}
