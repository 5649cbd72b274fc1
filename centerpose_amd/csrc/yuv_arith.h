// Limited-range YUV -> BGR of one pixel in 20-bit fixed point, once, for the host and the device: yuv_frames.hip converts the samples
// of a frame where the pre-process loads its taps, cp_yuv_to_bgr_host applies the same statements on the CPU (what a test pins).
// A matrix is six ints, coef = (CY, CVR, CVG, CUG, CUB, YOFF), every entry round(k * 2^20):
//     "bt601"  (1220542, 1673527, -852492, -409993, 2116026, 16)      1.164, 1.596, -0.813, -0.391, 2.018
//     "bt709"  (1220542, 1880097, -558891, -223347, 2214593, 16)      1.164, 1.793, -0.533, -0.213, 2.112
// "bt601" restates cv2.cvtColor(COLOR_YUV2BGR_NV12): the same constants, rounding term and shift.  int32 throughout, arithmetic right
// shifts; yf_coef_fits is the condition under which no intermediate can overflow.
#pragma once

#define YF_SHIFT 20

struct YfCoef { int cy, cvr, cvg, cug, cub, yoff; };

__host__ __device__ inline int yf_clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// (Y, U, V) bytes -> bgr[0..2] = B, G, R
__host__ __device__ inline void yf_yuv_to_bgr(int Y, int U, int V, const YfCoef& k, int bgr[3])
{
    const int yy = Y - k.yoff;
    const int y = (yy < 0 ? 0 : yy) * k.cy;
    const int u = U - 128, v = V - 128;
    const int half = 1 << (YF_SHIFT - 1);
    bgr[2] = yf_clamp_u8((y + k.cvr * v + half) >> YF_SHIFT);
    bgr[1] = yf_clamp_u8((y + k.cvg * v + k.cug * u + half) >> YF_SHIFT);
    bgr[0] = yf_clamp_u8((y + k.cub * u + half) >> YF_SHIFT);
}

// CY > 0, 0 <= YOFF <= 255 and 255 * CY + 2^19 + 128 * max(|CVR|, |CVG| + |CUG|, |CUB|) < 2^31
inline bool yf_coef_fits(const int* c, const char** why)
{
    if (c[0] <= 0) { *why = "CY must be positive"; return false; }
    if (c[5] < 0 || c[5] > 255) { *why = "YOFF must lie in 0..255"; return false; }
    long long a = c[1] < 0 ? -(long long)c[1] : c[1];
    const long long g = (c[2] < 0 ? -(long long)c[2] : c[2]) + (c[3] < 0 ? -(long long)c[3] : c[3]);
    const long long b = c[4] < 0 ? -(long long)c[4] : c[4];
    if (g > a) a = g;
    if (b > a) a = b;
    if (255ll * c[0] + (1ll << (YF_SHIFT - 1)) + 128 * a >= (1ll << 31)) { *why = "the sums could overflow int32"; return false; }
    return true;
}
