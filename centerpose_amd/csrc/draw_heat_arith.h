// The rule of the heat-map overlay, once, for the host and the device: the network's heat maps (pred_hm, pred_hmhp) turned into a
// colour map and blended over the whole frame, as the reference's MultiPoseDetector.debug shows them (Debugger.gen_colormap /
// gen_colormap_hp, add_blend_img).  draw_heat.hip compiles these statements into its kernels, draw_heat_host.h into the sequential
// host painters (what a test pins).  The translation units are compiled with -ffp-contract=off: every float and double statement
// below is one rounded operation after the other.
//
// 1. Colour map, per image and map cell, from the C values v_c of that cell and the palette P[c] = (B, G, R):
//      m_k = max over c of (v_c * P[c][k]) in float32, starting from 0 and compared with '>': a NaN never wins, negatives give 0;
//      cm_k = min(255, (int)m_k).  With `invert` P[c][k] is replaced by 255 - P[c][k] and cm_k by 255 - cm_k (the white theme).
//    A cell is one dword: B | G << 8 | R << 16.
// 2. Position, per frame pixel (x, y), with the frame -> map matrix T (six doubles, row major), in double:
//      mx = T00 * x + T01 * y + T02 (left to right), clamped to [0, w - 1]; X = (long long)(mx * 256.0 + 0.5); ix = X >> 8, fx = X & 255,
//      ix1 = min(ix + 1, w - 1); my, iy, fy, iy1 the same with the second row of T and h.  Map cell (i, j) sits AT map coordinate (i, j),
//      where post_process puts a peak -- not at cv2.resize's half-pixel centres.  No pixel is skipped: outside the map the border repeats.
// 3. Sample, per component, integer: t0 = a * (256 - fx) + b * fx on row iy, t1 likewise on row iy1,
//      f = (t0 * (256 - fy) + t1 * fy + 32768) >> 16.
// 4. Blend: do_blend(p, f, opacity) of draw_overlay_arith.h on the three colour bytes of the pixel.
// 5. 8-bit 4:2:0 YUV frames: a fore colour (B, G, R) goes to (Y, U, V) by dh_bgr_to_yuv, the forward forms of draw.palette_to_yuv.  Luma
//    is blended per pixel; a chroma sample with the (U, V) of the component-wise rounded mean (sum + (n >> 1)) / n of the fore colours
//    of its n in {1, 2, 4} in-frame pixels.
#pragma once
#include "draw_overlay_arith.h"

#define DH_MAX_CHANNELS 32
#define DH_MAX_CELLS (1ll << 30)    // N * h * w of one call

// mirror of cp_draw_heat_style (include/centerpose_hip.h)
struct DhStyle {
    int channels;                   // how many palette entries are filled: C..32
    int opacity;                    // 1..256
    int invert;                     // 0 / 1
    unsigned char palette[DH_MAX_CHANNELS][4];      // bytes 0..2: (B, G, R) of channel c; byte 3 is not used
};
static_assert(sizeof(DhStyle) == 140, "cp_draw_heat_style is 140 bytes");

// step 1 for one component: the running maximum takes value v of a channel whose palette byte is p
DA_HD float dh_peak(float m, float v, int p, int invert)
{
    const float t = v * (float)(invert ? 255 - p : p);
    return t > m ? t : m;
}

// step 1, the end: the component's byte from its maximum (m >= 0 or +inf, never NaN)
DA_HD int dh_level(float m, int invert)
{
    const int c = m >= 255.0f ? 255 : (int)m;
    return invert ? 255 - c : c;
}

// step 1 for one cell: v[c * stride], c < C -> the cell's dword
DA_HD uint32_t dh_cell(const float* v, long long stride, int C, const DhStyle& st)
{
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float x = v[c * stride];
        m0 = dh_peak(m0, x, st.palette[c][0], st.invert);
        m1 = dh_peak(m1, x, st.palette[c][1], st.invert);
        m2 = dh_peak(m2, x, st.palette[c][2], st.invert);
    }
    return (uint32_t)dh_level(m0, st.invert) | ((uint32_t)dh_level(m1, st.invert) << 8) | ((uint32_t)dh_level(m2, st.invert) << 16);
}

// step 2 for one axis: the map coordinate t0 * x + t1 * y + t2 against a side of n cells -> the cell, its neighbour, the fraction
DA_HD void dh_axis(double t0, double t1, double t2, int x, int y, int n, int* i0, int* i1, int* f)
{
    double m = t0 * (double)x + t1 * (double)y + t2;
    m = m > 0.0 ? m : 0.0;                                     // a NaN goes to 0
    m = m < (double)(n - 1) ? m : (double)(n - 1);
    const long long q = (long long)(m * 256.0 + 0.5);
    *i0 = (int)(q >> 8);
    *f = (int)(q & 255);
    *i1 = *i0 + 1 < n ? *i0 + 1 : n - 1;
}

// steps 2 and 3 for one frame pixel: the colour map cm [h, w] of its image sampled at (x, y) -> c[0..2] = (B, G, R)
DA_HD void dh_sample(const uint32_t* cm, int h, int w, const double* T, int x, int y, int* c)
{
    int ix, ix1, fx, iy, iy1, fy;
    dh_axis(T[0], T[1], T[2], x, y, w, &ix, &ix1, &fx);
    dh_axis(T[3], T[4], T[5], x, y, h, &iy, &iy1, &fy);
    const uint32_t a = cm[(long long)iy * w + ix], b = cm[(long long)iy * w + ix1];
    const uint32_t d = cm[(long long)iy1 * w + ix], e = cm[(long long)iy1 * w + ix1];
    for (int k = 0; k < 3; ++k) {
        const int s = 8 * k;
        const int t0 = (int)((a >> s) & 255u) * (256 - fx) + (int)((b >> s) & 255u) * fx;
        const int t1 = (int)((d >> s) & 255u) * (256 - fx) + (int)((e >> s) & 255u) * fx;
        c[k] = (t0 * (256 - fy) + t1 * fy + 32768) >> 16;
    }
}

// step 5: (B, G, R) -> (Y, U, V), limited range, 8 fractional bits; matrix 0: BT.601, 1: BT.709.  Equal to draw.palette_to_yuv.
DA_HD void dh_bgr_to_yuv(int b, int g, int r, int matrix, int* yuv)
{
    if (matrix == 0) {
        yuv[0] = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16;
        yuv[1] = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128;
        yuv[2] = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128;
    } else {
        yuv[0] = ((47 * r + 157 * g + 16 * b + 128) >> 8) + 16;
        yuv[1] = ((-26 * r - 87 * g + 112 * b + 128) >> 8) + 128;
        yuv[2] = ((112 * r - 102 * g - 10 * b + 128) >> 8) + 128;
    }
}

// step 5 for one 2 x 2 block at (px, py), both even, of an H x W frame: luma[q] of the in-frame pixel q = 2 * dy + dx (others untouched)
// and the (U, V) its chroma sample is blended with; -> n, the number of in-frame pixels
DA_HD int dh_block_yuv(const uint32_t* cm, int h, int w, const double* T, int px, int py, int H, int W, int matrix, int* luma, int* uv)
{
    int sum[3] = {0, 0, 0}, n = 0;
    for (int q = 0; q < 4; ++q) {
        const int x = px + (q & 1), y = py + (q >> 1);
        if (x >= W || y >= H) continue;
        int c[3], t[3];
        dh_sample(cm, h, w, T, x, y, c);
        dh_bgr_to_yuv(c[0], c[1], c[2], matrix, t);
        luma[q] = t[0];
        sum[0] += c[0]; sum[1] += c[1]; sum[2] += c[2];
        ++n;
    }
    int t[3];
    dh_bgr_to_yuv((sum[0] + (n >> 1)) / n, (sum[1] + (n >> 1)) / n, (sum[2] + (n >> 1)) / n, matrix, t);
    uv[0] = t[1];
    uv[1] = t[2];
    return n;
}
