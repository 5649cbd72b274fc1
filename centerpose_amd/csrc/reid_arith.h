// The crop rule of the re-id stage, once, for the host and the device: which detection rows get an embedding, which pixels of the
// frame their crop covers, and the value of every pixel of the 3 x 128 x 64 network input.  reid_crops.hip compiles these
// statements into its kernels, reid_host.h into the sequential host twins (what a test pins).  Include from a translation unit
// compiled with -ffp-contract=off: the blend and the normalisation are written one rounding per operation.
//
// Box (demo/demo_main.py:185-190 -> demo/tracking/deep_sort.py:66-72): a row is float32[56] = [x1, y1, x2, y2, score, ...].  The
// four coordinates are clamped to +-2^30 and truncated toward zero (a NaN coordinate: the row is not selected); w = x2 - x1,
// h = y2 - y1; X1 = max(x1, 0), Y1 = max(y1, 0), X2 = min(X1 + w, W - 1), Y2 = min(Y1 + h, H - 1); the crop is rows Y1..Y2-1 and
// columns X1..X2-1 (the reference's slice: exclusive ends, after a clamp to W - 1 -- the last column and row are never reached).
// A row is selected iff score > vis_thresh (strict; a NaN score is not) and the crop has pixels (X2 > X1 and Y2 > Y1).
//
// Resize (cv2.resize(crop.astype(float32), (64, 128)), INTER_LINEAR: half-pixel centres, no antialiasing): along an axis of n source
// and N destination pixels, destination o samples at fx = (o + 0.5) * (n / N) - 0.5 in double; s = floor(fx), f = float32(fx - s);
// s < 0: tap 0 alone; s >= n - 1: tap n - 1 alone; otherwise taps s, s + 1 with the float32 weights (1 - f, f).  Taps never leave
// the crop.  The four 8-bit taps are blended horizontally, then vertically, in double, then rounded to float32.
// Normalise (demo/tracking/feature_extractor.py:15-22) in float32: (v * scale - mean[k]) / std[k].
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RA_HD __host__ __device__ inline
#else
#define RA_HD inline
#endif

#define RA_ROW 56           // floats per detection row
#define RA_OUT_H 128
#define RA_OUT_W 64
#define RA_COORD_MAX 1073741824      // 2^30
#define RA_MAX_CAP 4096
#define RA_MAX_ROWS (1 << 24)        // N * M: a slot entry n * M + m fits an int with room

struct RaBox { int x1, y1, x2, y2; };       // the crop: rows y1..y2-1, columns x1..x2-1

// (scale, mean, std) and the channel pairing: output channel k reads source channel (rgb ? 2 - k : k) of the frame's (B, G, R)
struct RaNorm { float scale, mean[3], sd[3]; int rgb; };

RA_HD bool ra_coord(float v, int* out)
{
    if (v != v) return false;
    *out = v < -(float)RA_COORD_MAX ? -RA_COORD_MAX : (v > (float)RA_COORD_MAX ? RA_COORD_MAX : (int)v);
    return true;
}

// the crop of one row inside an H x W frame; false: the row gets no embedding
RA_HD bool ra_select(const float* row, float vis_thresh, int H, int W, RaBox* box)
{
    if (!(row[4] > vis_thresh)) return false;
    int x1, y1, x2, y2;
    if (!ra_coord(row[0], &x1) || !ra_coord(row[1], &y1) || !ra_coord(row[2], &x2) || !ra_coord(row[3], &y2)) return false;
    const long long w = (long long)x2 - x1, h = (long long)y2 - y1;
    const long long X1 = x1 > 0 ? x1 : 0, Y1 = y1 > 0 ? y1 : 0;
    const long long X2 = X1 + w < W - 1 ? X1 + w : W - 1, Y2 = Y1 + h < H - 1 ? Y1 + h : H - 1;
    if (X2 <= X1 || Y2 <= Y1) return false;
    box->x1 = (int)X1; box->y1 = (int)Y1; box->x2 = (int)X2; box->y2 = (int)Y2;
    return true;
}

struct RaTap { int i0, i1; float f; };      // offsets inside the crop and the weight of i1

RA_HD RaTap ra_tap(int o, int n, int N)
{
    const double ratio = (double)n / (double)N;
    const double fx = ((double)o + 0.5) * ratio - 0.5;
    const double fl = floor(fx);
    int s = (int)fl;
    float f = (float)(fx - fl);
    RaTap t;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; t.i1 = s; } else { t.i1 = s + 1; }
    t.i0 = s;
    t.f = f;
    return t;
}

// the four taps (top-left, top-right, bottom-left, bottom-right) of one channel -> the blended float32
RA_HD float ra_blend(int p00, int p01, int p10, int p11, float fx, float fy)
{
    const double ax0 = (double)(1.f - fx), ax1 = (double)fx, ay0 = (double)(1.f - fy), ay1 = (double)fy;
    const double top = (double)p00 * ax0 + (double)p01 * ax1;
    const double bot = (double)p10 * ax0 + (double)p11 * ax1;
    return (float)(top * ay0 + bot * ay1);
}

RA_HD float ra_norm(float v, const RaNorm& nm, int k) { return (v * nm.scale - nm.mean[k]) / nm.sd[k]; }

// One output pixel (oy, ox) of the crop `b`: src.load(y, x, v) puts the frame's (B, G, R) bytes of pixel (y, x) into v[0..2];
// r[k] = output channel k.
template <class Src>
RA_HD void ra_pixel(const Src& src, const RaBox& b, int oy, int ox, const RaNorm& nm, float r[3])
{
    const RaTap tx = ra_tap(ox, b.x2 - b.x1, RA_OUT_W), ty = ra_tap(oy, b.y2 - b.y1, RA_OUT_H);
    int p00[3], p01[3], p10[3], p11[3];
    src.load(b.y1 + ty.i0, b.x1 + tx.i0, p00);
    src.load(b.y1 + ty.i0, b.x1 + tx.i1, p01);
    src.load(b.y1 + ty.i1, b.x1 + tx.i0, p10);
    src.load(b.y1 + ty.i1, b.x1 + tx.i1, p11);
    for (int k = 0; k < 3; ++k) {
        const int c = nm.rgb ? 2 - k : k;
        r[k] = ra_norm(ra_blend(p00[c], p01[c], p10[c], p11[c], tx.f, ty.f), nm, k);
    }
}
