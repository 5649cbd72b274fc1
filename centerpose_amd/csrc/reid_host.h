// Host side of the re-id crop stage: the descriptor mirrors, the argument checks shared by the device launchers and the host twins,
// and the sequential host twins themselves (cp_reid_select_rows_host / cp_reid_crop_frames_host / cp_reid_crop_yuv_frames_host,
// exported by reid_crops.hip).  Plain C++ over reid_arith.h and yuv_arith.h, no device code and no HIP header:
// tools/reid_host_fuzz.cpp compiles this file with the host compiler under AddressSanitizer / UBSan.  A failed check writes its
// message to `err` and returns 1.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include "reid_arith.h"
#if !defined(__HIPCC__)     // yuv_arith.h (under yuv_source.h) marks its functions for both sides; a host compiler knows neither word
#define __host__
#define __device__
#endif
#include "yuv_source.h"

// mirror of cp_frame_desc (include/centerpose_hip.h); the crops read base, the strides, ch_off, H and W
struct RhFrameDesc {
    const unsigned char* base;
    long long row_stride, pix_stride;
    long long ch_off[3];
    long long mid_off;
    int H, W, NH, NW;
    double mi[6];
    int slot, pad;
};
static_assert(sizeof(RhFrameDesc) == 128, "cp_frame_desc is 128 bytes");

// mirror of cp_yuv_frame_desc; the crops read the bases, the strides, H and W
struct RhYuvFrameDesc {
    const unsigned char* y_base;
    long long y_row, y_pix;
    const unsigned char* u_base;
    const unsigned char* v_base;
    long long c_row, c_pix;
    long long mid_off;
    int H, W, NH, NW;
    double mi[6];
    int slot, pad;
};
static_assert(sizeof(RhYuvFrameDesc) == 136, "cp_yuv_frame_desc is 136 bytes");

static_assert(sizeof(RaNorm) == 32, "cp_reid_norm is 32 bytes");

// the frame's (B, G, R) bytes of pixel (y, x)
struct RhStrided {
    const unsigned char* base;
    long long row, pix, off[3];
    RA_HD void load(int y, int x, int v[3]) const
    {
        const unsigned char* p = base + (long long)y * row + (long long)x * pix;
        v[0] = p[off[0]]; v[1] = p[off[1]]; v[2] = p[off[2]];
    }
};
RA_HD RhStrided rh_source(const RhFrameDesc& d)
{
    RhStrided s = {d.base, d.row_stride, d.pix_stride, {d.ch_off[0], d.ch_off[1], d.ch_off[2]}};
    return s;
}

// the same from YUV planes: yuv_source.h's sampler (nearest chroma, yuv_arith.h per source pixel, exactly as the pre-process converts its
// taps).  GENERAL = false: 8-bit 4:2:0, every frame of the call has format word 0; true: any format word.
template <bool GENERAL>
RA_HD YsSource<GENERAL> rh_yuv_source(const RhYuvFrameDesc& d, const YfCoef& k)
{
    return ys_source<GENERAL>(d, k);
}

#define RH_CHECK(cond, ...)                      \
    do {                                         \
        if (!(cond)) {                           \
            snprintf(err, errn, __VA_ARGS__);    \
            return 1;                            \
        }                                        \
    } while (0)

// what does not depend on the frames
inline int rh_check_call(const char* who, int N, int M, int cap, char* err, size_t errn)
{
    RH_CHECK(cap >= 1 && cap <= RA_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, RA_MAX_CAP);
    RH_CHECK(N >= 1, "%s: %d frames: at least one", who, N);
    RH_CHECK(N <= cap, "%s: %d frames for a capacity of %d: every frame needs a slot", who, N, cap);
    RH_CHECK(M >= 0, "%s: negative row count %d", who, M);
    RH_CHECK((long long)N * M <= RA_MAX_ROWS, "%s: %d x %d rows are too many for one call (at most %d)", who, N, M, RA_MAX_ROWS);
    return 0;
}

inline int rh_check_norm(const char* who, const RaNorm* nm, char* err, size_t errn)
{
    RH_CHECK(nm, "%s: null norm", who);
    RH_CHECK(nm->rgb == 0 || nm->rgb == 1, "%s: channel order flag %d is neither 0 (bgr) nor 1 (rgb)", who, nm->rgb);
    return 0;
}

inline int rh_check_frames(const char* who, const RhFrameDesc* t, int N, char* err, size_t errn)
{
    for (int n = 0; n < N; ++n) {
        const RhFrameDesc& d = t[n];
        RH_CHECK(d.base, "%s: frame %d: null base address", who, n);
        RH_CHECK(d.H > 0 && d.W > 0 && (long long)d.H * d.W < (1ll << 29), "%s: frame %d: bad size %d x %d", who, n, d.H, d.W);
        RH_CHECK(d.row_stride >= 0 && d.pix_stride >= 0 && d.ch_off[0] >= 0 && d.ch_off[1] >= 0 && d.ch_off[2] >= 0,
                 "%s: frame %d: negative stride or channel offset", who, n);
        long long ch_max = d.ch_off[0];
        if (d.ch_off[1] > ch_max) ch_max = d.ch_off[1];
        if (d.ch_off[2] > ch_max) ch_max = d.ch_off[2];
        const __int128 last = (__int128)(d.H - 1) * d.row_stride + (__int128)(d.W - 1) * d.pix_stride + ch_max;
        RH_CHECK(last < ((__int128)1 << 62), "%s: frame %d: strides address more than 2^62 bytes", who, n);
    }
    return 0;
}

inline int rh_check_yuv_frames(const char* who, const RhYuvFrameDesc* t, int N, const int* coef, char* err, size_t errn)
{
    RH_CHECK(coef, "%s: null coef", who);
    const char* why = "";
    RH_CHECK(yf_coef_fits(coef, &why), "%s: bad conversion matrix: %s", who, why);
    for (int n = 0; n < N; ++n) {
        const RhYuvFrameDesc& d = t[n];
        RH_CHECK(d.H > 0 && d.W > 0 && (long long)d.H * d.W < (1ll << 29), "%s: frame %d: bad size %d x %d", who, n, d.H, d.W);
        const char* bad = ys_check_format(d);
        RH_CHECK(!bad, "%s: frame %d: %s (format word pad = %d; y %p, u %p, v %p)", who, n, bad, d.pad, (const void*)d.y_base,
                 (const void*)d.u_base, (const void*)d.v_base);
    }
    return 0;
}

// the selection reads H and W only; of a YUV table it also refuses format words no crop would take
inline int rh_check_yuv_words(const char* who, const RhYuvFrameDesc* t, int N, char* err, size_t errn)
{
    for (int n = 0; n < N; ++n) {
        const char* bad = ys_check_word(t[n].pad);
        RH_CHECK(!bad, "%s: frame %d: format word pad = %d: %s", who, n, t[n].pad, bad);
    }
    return 0;
}

// HOST selection: slots[cap] (n * M + m of the first q = cap / N selected rows of frame n at n * q + 0, 1, ...; -1: unused),
// counts[N] (selected rows per frame, uncapped)
template <class Desc>
inline void rh_select(const Desc* table, int N, const float* rows, int M, float vis_thresh, int cap, int* slots, int* counts)
{
    const int q = cap / N;
    for (int s = 0; s < cap; ++s) slots[s] = -1;
    for (int n = 0; n < N; ++n) {
        int c = 0;
        for (int m = 0; m < M; ++m) {
            RaBox b;
            if (!ra_select(rows + ((size_t)n * M + m) * RA_ROW, vis_thresh, table[n].H, table[n].W, &b)) continue;
            if (c < q) slots[n * q + c] = n * M + m;
            ++c;
        }
        counts[n] = c;
    }
}

// HOST crops: out [cap, 3, 128, 64]; a slot that is unused, out of range or whose row is not selected is written as zeros
template <class Desc, class Make>
inline void rh_crop(const Desc* table, int N, const float* rows, int M, float vis_thresh, const int* slots, int cap, const RaNorm& nm,
                    float* out, Make make)
{
    const size_t plane = (size_t)RA_OUT_H * RA_OUT_W;
    for (int s = 0; s < cap; ++s) {
        float* o = out + (size_t)s * 3 * plane;
        const int idx = slots[s];
        RaBox b;
        if (idx < 0 || idx >= N * M || !ra_select(rows + (size_t)idx * RA_ROW, vis_thresh, table[idx / M].H, table[idx / M].W, &b)) {
            for (size_t i = 0; i < 3 * plane; ++i) o[i] = 0.f;
            continue;
        }
        const auto src = make(table[idx / M]);
        for (int oy = 0; oy < RA_OUT_H; ++oy)
            for (int ox = 0; ox < RA_OUT_W; ++ox) {
                float r[3];
                ra_pixel(src, b, oy, ox, nm, r);
                for (int k = 0; k < 3; ++k) o[k * plane + (size_t)oy * RA_OUT_W + ox] = r[k];
            }
    }
}

inline int rh_select_host(const void* table, int yuv, int N, const float* rows, int M, float vis_thresh, int cap, int* slots, int* counts,
                          char* err, size_t errn)
{
    const char* who = "reid_select_rows_host";
    if (int rc = rh_check_call(who, N, M, cap, err, errn)) return rc;
    RH_CHECK(table && slots && counts && (rows || M == 0), "%s: null pointer", who);
    if (yuv) {
        if (int rc = rh_check_yuv_words(who, (const RhYuvFrameDesc*)table, N, err, errn)) return rc;
        rh_select((const RhYuvFrameDesc*)table, N, rows, M, vis_thresh, cap, slots, counts);
    } else
        rh_select((const RhFrameDesc*)table, N, rows, M, vis_thresh, cap, slots, counts);
    return 0;
}

inline int rh_crop_frames_host(const RhFrameDesc* table, int N, const float* rows, int M, float vis_thresh, const int* slots, int cap,
                               const RaNorm* nm, float* out, char* err, size_t errn)
{
    const char* who = "reid_crop_frames_host";
    if (int rc = rh_check_call(who, N, M, cap, err, errn)) return rc;
    if (int rc = rh_check_norm(who, nm, err, errn)) return rc;
    RH_CHECK(table && slots && out && (rows || M == 0), "%s: null pointer", who);
    if (int rc = rh_check_frames(who, table, N, err, errn)) return rc;
    rh_crop(table, N, rows, M, vis_thresh, slots, cap, *nm, out, [](const RhFrameDesc& d) { return rh_source(d); });
    return 0;
}

inline int rh_crop_yuv_frames_host(const RhYuvFrameDesc* table, int N, const int* coef, const float* rows, int M, float vis_thresh,
                                   const int* slots, int cap, const RaNorm* nm, float* out, char* err, size_t errn)
{
    const char* who = "reid_crop_yuv_frames_host";
    if (int rc = rh_check_call(who, N, M, cap, err, errn)) return rc;
    if (int rc = rh_check_norm(who, nm, err, errn)) return rc;
    RH_CHECK(table && slots && out && (rows || M == 0), "%s: null pointer", who);
    if (int rc = rh_check_yuv_frames(who, table, N, coef, err, errn)) return rc;
    const YfCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    rh_crop(table, N, rows, M, vis_thresh, slots, cap, *nm, out, [&](const RhYuvFrameDesc& d) { return rh_yuv_source<true>(d, k); });
    return 0;
}
