// The z-buffer mesh rasteriser of the aligned faces, stated once for the kernels (face_render.hip) and the host twins
// (face_render_host.h): what render_texture, get_triangle_buffer and get_depth_image do per face in three nested Python loops
// (demo/face/utils/render.py:85-120, 239-287; render_app.py:35-40), and PRN.get_colors (demo/face/prnet.py:155-168).  Compile every
// user with -ffp-contract=off: the products and sums below are the reference's, one rounding each.
//
// Per slot: float32 vertices v[V][3] (the cells face_ind of the slot's position map, get_vertices), a triangle table tri[T][3] of vertex
// indices, an integer window (x0, y0) with one (h, w) per call.  Image pixel (r, c) of slot s is frame pixel (X, Y) = (x0[s] + c,
// y0[s] + r).  The reference clamps a triangle's box to the frame [0, w-1] x [0, h-1]; HERE THE BOX IS CLAMPED TO THE WINDOW, so the
// result equals the reference's render of any frame that contains the window, cropped to the window.
//
// Arithmetic: float64 on the float32 inputs converted to double -- how the reference computes when fed float64 vertices (its own are).
// Per triangle i, in this order (fr_setup):
//   1. skipped iff any of its nine coordinates is not finite;
//   2. depth d = (float)(((z0 + z1) + z2) / 3.0) + 0.0f  (-0 and +0 tie);
//   3. skipped iff !(d > -999999.0f), the reference's initial buffer;
//   4. box: umin = max(ceil(min x), x0), umax = min(floor(max x), x0 + w - 1), likewise v; compared in double, converted to int only
//      once clamped;
//   5. a pixel of the box is covered iff isPointInTri holds (render.py:17-41, fr_covers): v0 = p2 - p0, v1 = p1 - p0, v2 = P - p0, the
//      five dot products as a * a' + b * b', inverDeno = 0 when the determinant is 0 (a degenerate triangle covers its whole box: kept),
//      covered iff u >= 0 && v >= 0 && u + v < 1.
// Winner per pixel: the covering triangle with the largest d, among equal d the smallest i (the reference's sequential strict >), as
// ONE unsigned 64-bit key ordered(d) << 32 | (0xFFFFFFFF - i), 0 = no triangle: the winner is a pure maximum, whatever the arrival order.
// Outputs: tri (the winner's index, -1 for none) and image: per covered pixel (float)(((a0 + a1) + a2) / 3.0) of the winner's three
// vertex attributes, double inside; 0 where nothing covers.
//
// Vertex colours (fr_color_cell): x clamped to [0, W - 1], y to [0, H - 1], rounded half to even (np.round); a coordinate that is not
// finite gives no cell (the vertex is written as zeros).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FR_HD __host__ __device__ inline
#else
#define FR_HD inline
#endif

#define FR_MAX_CAP 256
#define FR_MIN_V 3
#define FR_MAX_V 65536
#define FR_MAX_T (1 << 22)
#define FR_MAX_SIDE 4096
#define FR_MAX_ORIGIN (1 << 20)
#define FR_MAX_C 4
#define FR_CELLS 65536              // cells of one 256 x 256 position map
#define FR_LANE_BOX 16              // a box of at most this many pixels is walked by the triangle's own lane

FR_HD bool fr_finite(float v) { return v - v == 0.f; }

FR_HD uint32_t fr_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// the usual monotone map of float bits: a < b <=> ordered(a) < ordered(b); never 0 for a number
FR_HD uint32_t fr_ordered(float f)
{
    const uint32_t u = fr_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

FR_HD uint64_t fr_key(float d, int i) { return ((uint64_t)fr_ordered(d) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i); }
FR_HD int fr_key_tri(uint64_t key) { return key ? (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu)) : -1; }

// A slot is rendered iff it is used (slots[s] >= 0) and its window's origin lies within +-2^20; the origin lies on the device, so it is
// checked where it is read, and a slot that fails is written like an unused one.
FR_HD bool fr_slot_used(const int* slots, const int* origin, int s)
{
    const int x0 = origin[2 * s], y0 = origin[2 * s + 1];
    return slots[s] >= 0 && x0 >= -FR_MAX_ORIGIN && x0 <= FR_MAX_ORIGIN && y0 >= -FR_MAX_ORIGIN && y0 <= FR_MAX_ORIGIN;
}

// one vertex attribute of a triangle: tri_tex / tri_depth of render.py:99-100
FR_HD float fr_mean3(float a0, float a1, float a2) { return (float)((((double)a0 + (double)a1) + (double)a2) / 3.0); }

// A triangle ready to be walked: its depth, its box inside the window (frame coordinates) and isPointInTri's per-triangle terms
struct FrTri {
    float d;
    int umin, umax, vmin, vmax;
    double px, py, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv;
};

FR_HD double fr_min3(double a, double b, double c) { const double m = a < b ? a : b; return m < c ? m : c; }
FR_HD double fr_max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }

// steps 1-4 and the terms of step 5 that do not depend on the pixel; false: the triangle touches no pixel
FR_HD bool fr_setup(const float* p0, const float* p1, const float* p2, int x0, int y0, int h, int w, FrTri* t)
{
    for (int k = 0; k < 3; ++k)
        if (!(fr_finite(p0[k]) && fr_finite(p1[k]) && fr_finite(p2[k]))) return false;
    t->d = fr_mean3(p0[2], p1[2], p2[2]) + 0.0f;
    if (!(t->d > -999999.0f)) return false;
    const double ax = p0[0], ay = p0[1], bx = p1[0], by = p1[1], cx = p2[0], cy = p2[1];
    double lo = ceil(fr_min3(ax, bx, cx)), hi = floor(fr_max3(ax, bx, cx));
    if (lo < (double)x0) lo = (double)x0;
    if (hi > (double)(x0 + w - 1)) hi = (double)(x0 + w - 1);
    if (hi < lo) return false;
    t->umin = (int)lo; t->umax = (int)hi;
    lo = ceil(fr_min3(ay, by, cy)); hi = floor(fr_max3(ay, by, cy));
    if (lo < (double)y0) lo = (double)y0;
    if (hi > (double)(y0 + h - 1)) hi = (double)(y0 + h - 1);
    if (hi < lo) return false;
    t->vmin = (int)lo; t->vmax = (int)hi;
    t->px = ax; t->py = ay;
    t->v0x = cx - ax; t->v0y = cy - ay;
    t->v1x = bx - ax; t->v1y = by - ay;
    t->dot00 = t->v0x * t->v0x + t->v0y * t->v0y;
    t->dot01 = t->v0x * t->v1x + t->v0y * t->v1y;
    t->dot11 = t->v1x * t->v1x + t->v1y * t->v1y;
    const double det = t->dot00 * t->dot11 - t->dot01 * t->dot01;
    t->inv = det == 0.0 ? 0.0 : 1.0 / det;
    return true;
}

// isPointInTri for frame pixel (X, Y)
FR_HD bool fr_covers(const FrTri& t, int X, int Y)
{
    const double v2x = (double)X - t.px, v2y = (double)Y - t.py;
    const double dot02 = t.v0x * v2x + t.v0y * v2y;
    const double dot12 = t.v1x * v2x + t.v1y * v2y;
    const double u = (t.dot11 * dot02 - t.dot01 * dot12) * t.inv;
    const double v = (t.dot00 * dot12 - t.dot01 * dot02) * t.inv;
    return u >= 0.0 && v >= 0.0 && u + v < 1.0;
}

// the three vertices of triangle i of a slot, straight from its map: map [65536][3], face_ind [V], tri [T][3]
FR_HD void fr_gather(const float* map, const int* face_ind, const int* tri, int i, const float* p[3])
{
    for (int k = 0; k < 3; ++k) p[k] = map + (size_t)face_ind[tri[3 * (size_t)i + k]] * 3;
}

// key -> tri and image of one pixel; attrs: the slot's [V][C], or null: the vertices' z (C = 1)
FR_HD void fr_resolve(uint64_t key, const float* map, const int* face_ind, const int* tri, const float* attrs, int C, int* out_tri,
                      float* out_image)
{
    const int i = fr_key_tri(key);
    *out_tri = i;
    if (i < 0) {
        for (int c = 0; c < C; ++c) out_image[c] = 0.f;
        return;
    }
    const int a = tri[3 * (size_t)i], b = tri[3 * (size_t)i + 1], e = tri[3 * (size_t)i + 2];
    if (!attrs) {
        out_image[0] = fr_mean3(map[(size_t)face_ind[a] * 3 + 2], map[(size_t)face_ind[b] * 3 + 2], map[(size_t)face_ind[e] * 3 + 2]);
        return;
    }
    for (int c = 0; c < C; ++c) out_image[c] = fr_mean3(attrs[(size_t)a * C + c], attrs[(size_t)b * C + c], attrs[(size_t)e * C + c]);
}

// one axis of get_colors: clamp to [0, n - 1], round half to even -> the cell, or -1 for a coordinate that is not finite
FR_HD int fr_color_cell(float x, int n)
{
    if (!fr_finite(x)) return -1;
    double v = (double)x;
    if (v < 0.0) v = 0.0;
    if (v > (double)(n - 1)) v = (double)(n - 1);
    return (int)rint(v);
}

// the colours of one vertex: the frame's (B, G, R) at its cell, or zeros
template <class Src>
FR_HD void fr_color(const Src& src, int H, int W, const float* p, float out[3])
{
    const int cx = fr_color_cell(p[0], W), cy = fr_color_cell(p[1], H);
    out[0] = out[1] = out[2] = 0.f;
    if (cx < 0 || cy < 0) return;
    int bgr[3];
    src.load(cy, cx, bgr);
    out[0] = (float)bgr[0]; out[1] = (float)bgr[1]; out[2] = (float)bgr[2];
}
