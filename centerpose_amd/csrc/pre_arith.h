// The 8-bit fixed-point arithmetic of the batched pre-process, once: cv2.resize (INTER_LINEAR) and cv2.warpAffine + normalise per
// destination pixel, statement for statement those of prepost.hip (resize_u8_kernel, preprocess_kernel).  batch_stages.hip reads its
// sources from one packed staging buffer (BsPacked), frame_sources.hip reads every frame in place through a pointer and strides
// (BsStrided), yuv_frames.hip converts (Y, U, V) samples to the three bytes where the taps are loaded (YsSource, yuv_source.h); the statements
// between the loads are the same functions, so all are bit-identical to the per-image calls.  Include from a translation unit
// compiled with -ffp-contract=off.
#pragma once
#include "common.h"

#define BS_THREADS 256

// A source image: load(y, x, v) puts the three bytes of pixel (y, x), in network channel order (k = 0, 1, 2), into v[0..2].
// packed uint8 [H,W,3], channels in network order
struct BsPacked {
    const unsigned char* img;
    int W;
    __device__ __forceinline__ void load(int y, int x, int v[3]) const
    {
        const unsigned char* p = img + ((size_t)y * W + x) * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
};

// any layout: base + y * row + x * pix + off[k] (packed BGR / RGB, BGRA / RGBA, planar CHW, crops, padded rows, expanded views)
struct BsStrided {
    const unsigned char* base;
    long long row, pix, off[3];
    __device__ __forceinline__ void load(int y, int x, int v[3]) const
    {
        const unsigned char* p = base + (long long)y * row + (long long)x * pix;
        v[0] = p[off[0]]; v[1] = p[off[1]]; v[2] = p[off[2]];
    }
};

__device__ __forceinline__ int bs_sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// resize_taps of prepost.hip
__device__ __forceinline__ void bs_resize_taps(int d, double scale, int n, bool vertical, int& i0, int& i1, int& w0, int& w1)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (!vertical) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n - 1) { f = 0.f; s = n - 1; }
    }
    w1 = bs_sat_short(__float2int_rn(f * 2048.f));
    w0 = bs_sat_short(__float2int_rn((1.f - f) * 2048.f));
    i0 = min(max(s, 0), n - 1);
    i1 = min(max(s + 1, 0), n - 1);
}

// one destination pixel (dy, dx) of resize_u8_kernel (prepost.hip): the three channels, in network order, to dst[0..2]
template <class Src>
__device__ __forceinline__ void bs_resize_pixel(const Src& src, int H, int W, double scale_x, double scale_y, int dx, int dy,
                                                unsigned char* __restrict__ dst)
{
    int x0, x1, a0, a1, y0, y1, b0, b1;
    bs_resize_taps(dx, scale_x, W, false, x0, x1, a0, a1);
    bs_resize_taps(dy, scale_y, H, true, y0, y1, b0, b1);
    int p00[3], p01[3], p10[3], p11[3];
    src.load(y0, x0, p00);
    src.load(y0, x1, p01);
    src.load(y1, x0, p10);
    src.load(y1, x1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = p00[c] * a0 + p01[c] * a1;
        const int S1 = p10[c] * a0 + p11[c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        dst[c] = (unsigned char)min(max(v, 0), 255);
    }
}

struct BsNorm { float mean[3], sd[3]; };

// one destination pixel of preprocess_kernel (prepost.hip): the three normalised channels
template <class Src>
__device__ __forceinline__ void bs_warp_pixel(const Src& src, int H, int W, const double* m, int ox, int oy, const BsNorm& nm, float r[3])
{
    const int adelta = (int)__double2ll_rn(m[0] * (double)ox * 1024.0);
    const int bdelta = (int)__double2ll_rn(m[3] * (double)ox * 1024.0);
    const int X0 = (int)__double2ll_rn((m[1] * (double)oy + m[2]) * 1024.0) + 16;
    const int Y0 = (int)__double2ll_rn((m[4] * (double)oy + m[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = bs_sat_short(X >> 5), sy = bs_sat_short(Y >> 5);
    const int fx = X & 31, fy = Y & 31;
    int w[4] = {(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32};
    if (w[0] > 32767) w[0] = 32767;
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int yy = sy + (t >> 1), xx = sx + (t & 1);
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;      // constant border, value 0
        int p[3];
        src.load(yy, xx, p);
        acc[0] += w[t] * p[0]; acc[1] += w[t] * p[1]; acc[2] += w[t] * p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int u8 = min(max((acc[c] + (1 << 14)) >> 15, 0), 255);
        r[c] = (float)((((double)u8 / 255.0) - (double)nm.mean[c]) / (double)nm.sd[c]);
    }
}

// The OH x OW destination pixels of one image, grid-strided over blockIdx.x: warp + normalise + HWC->CHW into plane block `o`, and
// the mirrored twin into `tw` when flip.  VEC (OW % 4 == 0, 16-B aligned output): a lane owns four consecutive ox and stores one
// float4 per channel plane, and the reversed float4 into the twin's plane (flip_merge_pairs_kernel<vec4>'s shape: OW - 4 - ox0 is a
// multiple of 4 as well).
template <bool VEC, class Src>
__device__ __forceinline__ void bs_warp_image(const Src& src, int H, int W, const double* m, float* __restrict__ o, float* __restrict__ tw,
                                              int OH, int OW, const BsNorm& nm, int flip)
{
    const size_t total = (size_t)OH * OW;
    const int Wq = VEC ? OW >> 2 : OW, items = OH * Wq;
    for (int i = blockIdx.x * BS_THREADS + threadIdx.x; i < items; i += gridDim.x * BS_THREADS) {
        const int oy = i / Wq, xq = i - oy * Wq;
        if (VEC) {
            const int ox0 = 4 * xq;
            float r[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) bs_warp_pixel(src, H, W, m, ox0 + k, oy, nm, r[k]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                *reinterpret_cast<float4*>(o + c * total + (size_t)oy * OW + ox0) = make_float4(r[0][c], r[1][c], r[2][c], r[3][c]);
                if (flip)
                    *reinterpret_cast<float4*>(tw + c * total + (size_t)oy * OW + (OW - 4 - ox0)) = make_float4(r[3][c], r[2][c], r[1][c], r[0][c]);
            }
        } else {
            float r[3];
            bs_warp_pixel(src, H, W, m, xq, oy, nm, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[c * total + (size_t)oy * OW + xq] = r[c];
                if (flip) tw[c * total + (size_t)oy * OW + (OW - 1 - xq)] = r[c];
            }
        }
    }
}
