// The drawing rule of draw_tracks, once, for the host and the device: the three primitives of a track item -- its box, the filled bar
// at the box's top-left corner, the label written on the bar -- and the 5 x 7 font of the label.  draw_tracks.hip compiles these
// statements into its kernel, draw_tracks_host.h into the sequential host painters (what a test pins).  Integer-only.
//
// An item is a box (x0, y0) <= (x1, y1) with coordinates in [-16384, 16383], a colour for box and bar, a colour for the text and up to
// 16 glyph indices.  With the call's box thickness T (0..64) and font scale s (0..8; 0: no bar and no text), tw = 6 s nchars - s and
// th = 7 s, the primitives in paint order (the paint index is item * 3 + primitive):
//   0 the box   : the box rule of draw_arith.h (da_covers, primitive 0) with thickness T
//   1 the bar   : the closed rectangle [x0, x0 + tw + 3] x [y0, y0 + th + 4]; absent when nchars = 0 or s = 0
//   2 the text  : dx = x - (x0 + 2), dy = y - (y0 + 2); 0 <= dx < tw, 0 <= dy < th, u = (dx mod 6s) / s < 5 and bit (4 - u) of
//                 font[glyph[dx / 6s]][dy / s] set; absent with the bar
// tw <= 760 and th <= 56, so every value stays far below 2^31.  A glyph cell is 6 s wide: five columns and one of spacing, none after
// the last character.
#pragma once
#include "draw_arith.h"

#define DT_PRIMS 3
#define DT_MAX_CHARS 16
#define DT_MAX_SCALE 8
#define DT_GLYPHS 42
#define DT_GLYPH_ROWS 7
#define DT_MAX_ITEMS (1 << 24)      // N * Kmax: a paint index, item * 3 + primitive, fits an int

// mirror of cp_draw_track_item (include/centerpose_hip.h)
struct DtItem {
    int x0, y0, x1, y1;                 // corners sorted, each in [-16384, 16383]
    unsigned char color[4];             // bytes 0..2: what the box and the bar store; byte 3 is not used
    unsigned char text_color[4];        // bytes 0..2: what the text stores
    int nchars;                         // 0..16
    unsigned char glyph[DT_MAX_CHARS];  // indices into the font, the first nchars are read
};
static_assert(sizeof(DtItem) == 44, "cp_draw_track_item is 44 bytes");

// Row r (0 = top) of glyph g: bit 4 is the leftmost of the five columns.  Glyph order: 0-9, A-Z, space, # - . : _
DA_HD unsigned dt_font_row(int g, int r)
{
    constexpr unsigned char F[DT_GLYPHS][DT_GLYPH_ROWS] = {
        {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E},   // 0
        {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},   // 1
        {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},   // 2
        {0x1E, 0x01, 0x01, 0x0E, 0x01, 0x01, 0x1E},   // 3
        {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02},   // 4
        {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},   // 5
        {0x0E, 0x10, 0x10, 0x1E, 0x11, 0x11, 0x0E},   // 6
        {0x1F, 0x01, 0x02, 0x04, 0x04, 0x08, 0x08},   // 7
        {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},   // 8
        {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x01, 0x0E},   // 9
        {0x0E, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11},   // A
        {0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E},   // B
        {0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E},   // C
        {0x1E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x1E},   // D
        {0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F},   // E
        {0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10},   // F
        {0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0E},   // G
        {0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11},   // H
        {0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E},   // I
        {0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C},   // J
        {0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11},   // K
        {0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F},   // L
        {0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11},   // M
        {0x11, 0x19, 0x15, 0x13, 0x11, 0x11, 0x11},   // N
        {0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E},   // O
        {0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10},   // P
        {0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D},   // Q
        {0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11},   // R
        {0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E},   // S
        {0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04},   // T
        {0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E},   // U
        {0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04},   // V
        {0x11, 0x11, 0x11, 0x15, 0x15, 0x1B, 0x11},   // W
        {0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11},   // X
        {0x11, 0x11, 0x0A, 0x04, 0x04, 0x04, 0x04},   // Y
        {0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F},   // Z
        {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00},   // space
        {0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A},   // #
        {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00},   // -
        {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C},   // .
        {0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00},   // :
        {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x1F},   // _
    };
    return (g >= 0 && g < DT_GLYPHS) ? F[g][r] : 0u;            // the launchers refuse an index outside the table; never read past it
}

// the glyph index of a character of the set, -1 for any other (lower case is folded by the caller)
DA_HD int dt_glyph_index(int ch)
{
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'A' && ch <= 'Z') return 10 + (ch - 'A');
    switch (ch) {
    case ' ': return 36;
    case '#': return 37;
    case '-': return 38;
    case '.': return 39;
    case ':': return 40;
    case '_': return 41;
    default: return -1;
    }
}

DA_HD bool dt_has_label(const DtItem& it, int s) { return s > 0 && it.nchars > 0; }
DA_HD int dt_text_w(const DtItem& it, int s) { return 6 * s * it.nchars - s; }
DA_HD int dt_text_h(int s) { return 7 * s; }

// the bounding box of what an item can cover: the union of its box and its bar
DA_HD void dt_bounds(const DtItem& it, int s, int* x0, int* y0, int* x1, int* y1)
{
    *x0 = it.x0; *y0 = it.y0; *x1 = it.x1; *y1 = it.y1;
    if (dt_has_label(it, s)) {
        const int bx = it.x0 + dt_text_w(it, s) + 3, by = it.y0 + dt_text_h(s) + 4;
        if (bx > *x1) *x1 = bx;
        if (by > *y1) *y1 = by;
    }
}

// whether primitive l (0 box, 1 bar, 2 text) of an item covers pixel (x, y)
DA_HD bool dt_covers(const DtItem& it, int l, int T, int s, int x, int y)
{
    if (l == 0) {
        const DaPrim box = {it.x0, it.y0, it.x1, it.y1};
        return da_covers(box, 0, T, -1, -1, x, y);
    }
    if (!dt_has_label(it, s)) return false;
    const int tw = dt_text_w(it, s), th = dt_text_h(s);
    if (l == 1) return x >= it.x0 && x <= it.x0 + tw + 3 && y >= it.y0 && y <= it.y0 + th + 4;
    const int dx = x - (it.x0 + 2), dy = y - (it.y0 + 2);
    if (dx < 0 || dx >= tw || dy < 0 || dy >= th) return false;
    const int cell = dx / (6 * s), u = (dx - cell * 6 * s) / s;
    if (u >= 5 || cell >= DT_MAX_CHARS) return false;           // cell < nchars <= 16 for a checked item
    return (dt_font_row(it.glyph[cell], dy / s) >> (4 - u)) & 1u;
}

// the last primitive of one item that covers (x, y); -1: none
DA_HD int dt_item_winner(const DtItem& it, int T, int s, int x, int y)
{
    for (int l = DT_PRIMS - 1; l >= 0; --l)
        if (dt_covers(it, l, T, s, x, y)) return l;
    return -1;
}
