// The drawing rule of draw_results, once, for the host and the device: which primitives a detection row has and which pixels each of
// them covers.  draw_results.hip compiles these statements into its two kernels, draw_host.h into the sequential host painters (what
// a test pins).  Integer-only after the coordinate conversion; every product is taken in 64 bits.
//
// A row is float32[56]: box 0:4 (x0, y0, x1, y1), score 4, joints 5:39 as (x, y) pairs, joint scores 39:56.  It is live iff
// row[4] > vis_thresh (a NaN score is not).  A coordinate that is not finite (tested on the float's bits) kills the primitive it
// belongs to; any other is clamped to [-16384, 16383] and truncated toward zero.  Frames are at most 16384 x 16384, so a pixel
// differs from a coordinate by less than 2^15, a dot or cross product stays below 2^32 in magnitude and a squared cross product
// below 2^63.
//
// The 36 primitives of a row in paint order (the index is also the palette entry): 0 the box, 1..18 the limbs, 19..35 the joints.
//   joint at P, radius R      : |p - P|^2 <= k, k = R^2 + R                        (R = 0, 1, 2, 3: 1, 9, 21, 37 pixels)
//   limb P -> Q, radius R     : a = p - P, d = Q - P, L2 = d.d, t = a.d;  L2 = 0 or t <= 0: a.a <= k;  t >= L2: |p - Q|^2 <= k;
//                               otherwise (a x d)^2 <= k * L2
//   box, thickness T          : corners sorted; inside the closed rectangle and less than T pixels from one of its sides
// k < (R + 1)^2, so a covered pixel is within R of the primitive's bounding box in x and in y: the early rejection of da_covers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DA_HD __host__ __device__ inline
#else
#define DA_HD inline
#endif

#define DA_PRIMS 36
#define DA_LIMBS 18
#define DA_JOINTS 17
#define DA_ROW 56
#define DA_MAX_SIDE 16384
#define DA_MAX_REACH 64

// mirror of cp_draw_style (include/centerpose_hip.h)
struct DaStyle {
    int box_thickness;      // 0..64, 0: no box
    int limb_radius;        // -1: no limbs, 1..64
    int joint_radius;       // -1: no joints, 0..64
    unsigned char palette[DA_PRIMS][4];     // bytes 0..2 of entry l: what primitive l stores; byte 3 is not used
};
static_assert(sizeof(DaStyle) == 156, "cp_draw_style is 156 bytes");

// mirror of cp_draw_id_palette: a row whose id is >= 0 paints all of its primitives in colors[id % count]
#define DA_MAX_ID_COLORS 64
struct DaIdPalette {
    int count;              // 1..64
    unsigned char colors[DA_MAX_ID_COLORS][4];      // bytes 0..2 as in DaStyle's palette; byte 3 is not used
};
static_assert(sizeof(DaIdPalette) == 260, "cp_draw_id_palette is 260 bytes");

// what primitive l of a row stores: the style's colour, or with row ids the identity colour of a row whose id is >= 0
DA_HD const unsigned char* da_color(const DaStyle& st, const DaIdPalette* idp, int id, int l)
{
    return (idp && id >= 0) ? idp->colors[id % idp->count] : st.palette[l];
}

// box: (x0, y0) <= (x1, y1), sorted; limb: P = (x0, y0), Q = (x1, y1); joint: P = Q = (x0, y0)
struct DaPrim { int x0, y0, x1, y1; };

DA_HD bool da_finite(float v)
{
    union { float f; uint32_t u; } c;
    c.f = v;
    return (c.u & 0x7f800000u) != 0x7f800000u;
}

DA_HD bool da_coord(float v, int* out)
{
    if (!da_finite(v)) return false;
    *out = v < -16384.f ? -16384 : (v > 16383.f ? 16383 : (int)v);
    return true;
}

DA_HD bool da_live(const float* row, float vis_thresh) { return row[4] > vis_thresh; }

DA_HD void da_limb_joints(int i, int* a, int* b)
{
    constexpr unsigned char A[DA_LIMBS] = {0, 0, 1, 2, 3, 4, 5, 5, 7, 6, 8, 5, 6, 11, 11, 13, 12, 14};
    constexpr unsigned char B[DA_LIMBS] = {1, 2, 3, 4, 5, 6, 6, 7, 9, 8, 10, 11, 12, 12, 13, 15, 14, 16};
    *a = A[i];
    *b = B[i];
}

// How far primitive l paints beyond its corner points under the style; < 0: the style does not paint it.
DA_HD int da_reach(int box_thickness, int limb_radius, int joint_radius, int l)
{
    if (l == 0) return box_thickness > 0 ? 0 : -1;
    if (l <= DA_LIMBS) return limb_radius >= 1 ? limb_radius : -1;
    return joint_radius;
}

DA_HD bool da_joint_point(const float* row, int j, int* x, int* y)
{
    if (!(row[39 + j] > 0.f)) return false;
    const bool okx = da_coord(row[5 + 2 * j], x), oky = da_coord(row[6 + 2 * j], y);
    return okx && oky;
}

// primitive l of a live row -> whether it exists, and its points
DA_HD bool da_build(const float* row, int l, DaPrim* p)
{
    if (l == 0) {
        int x0, y0, x1, y1;
        const bool a = da_coord(row[0], &x0), b = da_coord(row[1], &y0), c = da_coord(row[2], &x1), d = da_coord(row[3], &y1);
        if (!(a && b && c && d)) return false;
        p->x0 = x0 < x1 ? x0 : x1; p->x1 = x0 < x1 ? x1 : x0;
        p->y0 = y0 < y1 ? y0 : y1; p->y1 = y0 < y1 ? y1 : y0;
        return true;
    }
    if (l <= DA_LIMBS) {
        int ja, jb;
        da_limb_joints(l - 1, &ja, &jb);
        const bool a = da_joint_point(row, ja, &p->x0, &p->y0), b = da_joint_point(row, jb, &p->x1, &p->y1);
        return a && b;
    }
    const bool a = da_joint_point(row, l - 1 - DA_LIMBS, &p->x0, &p->y0);
    p->x1 = p->x0; p->y1 = p->y0;
    return a;
}

// the bounding box of what primitive p (index l, reach r >= 0) can cover
DA_HD void da_bounds(const DaPrim& p, int r, int* x0, int* y0, int* x1, int* y1)
{
    *x0 = (p.x0 < p.x1 ? p.x0 : p.x1) - r; *x1 = (p.x0 < p.x1 ? p.x1 : p.x0) + r;
    *y0 = (p.y0 < p.y1 ? p.y0 : p.y1) - r; *y1 = (p.y0 < p.y1 ? p.y1 : p.y0) + r;
}

DA_HD bool da_disc(long long ax, long long ay, long long k) { return ax * ax + ay * ay <= k; }

// whether primitive p of index l covers pixel (x, y); the style paints it (da_reach >= 0)
DA_HD bool da_covers(const DaPrim& p, int l, int box_thickness, int limb_radius, int joint_radius, int x, int y)
{
    if (l == 0) {
        if (x < p.x0 || x > p.x1 || y < p.y0 || y > p.y1) return false;
        const int T = box_thickness;
        return x - p.x0 < T || p.x1 - x < T || y - p.y0 < T || p.y1 - y < T;
    }
    const int R = l <= DA_LIMBS ? limb_radius : joint_radius;
    int bx0, by0, bx1, by1;
    da_bounds(p, R, &bx0, &by0, &bx1, &by1);
    if (x < bx0 || x > bx1 || y < by0 || y > by1) return false;
    const long long k = (long long)R * R + R;
    const long long ax = x - p.x0, ay = y - p.y0;
    if (l > DA_LIMBS) return da_disc(ax, ay, k);
    const long long dx = p.x1 - p.x0, dy = p.y1 - p.y0;
    const long long L2 = dx * dx + dy * dy, t = ax * dx + ay * dy;
    if (L2 == 0 || t <= 0) return da_disc(ax, ay, k);
    if (t >= L2) return da_disc(x - p.x1, y - p.y1, k);
    const long long cr = ax * dy - ay * dx;
    return cr * cr <= k * L2;
}

// the last primitive of one row that covers (x, y), scanning from the back over the primitives in `mask`; -1: none
DA_HD int da_row_winner(const DaPrim* prims, uint64_t mask, int box_thickness, int limb_radius, int joint_radius, int x, int y)
{
    for (int l = DA_PRIMS - 1; l >= 0; --l)
        if (((mask >> l) & 1) && da_covers(prims[l], l, box_thickness, limb_radius, joint_radius, x, y)) return l;
    return -1;
}
