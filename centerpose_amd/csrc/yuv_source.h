// One YUV frame as a source of pixels, once, for the host and the device: the sampler every reader of cp_yuv_frame_desc shares
// (yuv_frames.hip, reid_crops.hip, the host twins of reid_host.h), the meaning of the descriptor's trailing format word, the 16-bit
// conversion rule next to yuv_arith.h's 8-bit one, and the checks of a descriptor that depend on its format.  Plain C++ over
// yuv_arith.h: tools/yuv_source_host_fuzz.cpp compiles this file with the host compiler under AddressSanitizer / UBSan.
//
// Format word (cp_yuv_frame_desc.pad), 0 = 8-bit 4:2:0 as before the word had a meaning:
//     bit 0  chroma not subsampled horizontally         bit 2  16-bit samples, little-endian, strides still in bytes
//     bit 1  chroma not subsampled vertically            bit 3  no chroma planes (grey): U = V = mid-scale
// Y(r, c) is the sample at y_base + r * y_row + c * y_pix, U(r, c) the sample at u_base + (r >> sy) * c_row + (c >> sx) * c_pix, V(r, c)
// the same from v_base: nearest chroma, no interpolation; (sx, sy) = (1, 1) for 4:2:0, (1, 0) for 4:2:2, (0, 0) for 4:4:4.
//
// 16-bit samples are used as stored, s in [0, 65535] (P010: ten bits in the MSBs, whatever the low six bits hold counts), in int64:
//     yy = max(Y - 256 * YOFF, 0);  u = U - 32768;  v = V - 32768
//     R = clamp((CY * yy + CVR * v + 2^27) >> 28, 0, 255)       G: CVG * v + CUG * u       B: CUB * u
// so that a frame holding x << 8 converts to exactly the bytes yf_yuv_to_bgr gives for x.
#pragma once
#include "yuv_arith.h"

#if defined(__HIPCC__)
#define YS_HD __host__ __device__ __forceinline__
#else
#define YS_HD inline
#endif

#define YS_FULL_X 1
#define YS_FULL_Y 2
#define YS_16BIT 4
#define YS_GREY 8
#define YS_FORMAT_MAX 15

YS_HD int ys_clamp_u8(long long v) { return v < 0 ? 0 : (v > 255 ? 255 : (int)v); }

// (Y, U, V) 16-bit container values -> bgr[0..2] = B, G, R bytes
YS_HD void yf_yuv16_to_bgr(int Y, int U, int V, const YfCoef& k, int bgr[3])
{
    const int yy = Y - 256 * k.yoff;
    const long long y = (long long)(yy < 0 ? 0 : yy) * k.cy;
    const long long u = U - 32768, v = V - 32768;
    const long long half = 1ll << (YF_SHIFT + 7);
    bgr[2] = ys_clamp_u8((y + k.cvr * v + half) >> (YF_SHIFT + 8));
    bgr[1] = ys_clamp_u8((y + k.cvg * v + k.cug * u + half) >> (YF_SHIFT + 8));
    bgr[0] = ys_clamp_u8((y + k.cub * u + half) >> (YF_SHIFT + 8));
}

YS_HD int ys_sx(int fmt) { return (fmt & YS_FULL_X) ? 0 : 1; }
YS_HD int ys_sy(int fmt) { return (fmt & YS_FULL_Y) ? 0 : 1; }

// one 16-bit sample: ONE 2-byte load (the address is even: ys_check_format), never a 4-byte load of an interleaved pair
YS_HD int ys_load16(const unsigned char* p)
{
    unsigned short s;
    __builtin_memcpy(&s, p, 2);
    return s;
}

// load(r, c, bgr): the B, G, R bytes of pixel (r, c).  GENERAL = false is the 8-bit 4:2:0 reader (format word 0): three byte loads per
// tap, whatever the plane layout, and no look at the format.  GENERAL = true reads any format; the word is uniform over a frame.
template <bool GENERAL>
struct YsSource {
    const unsigned char *y, *u, *v;
    long long y_row, y_pix, c_row, c_pix;
    YfCoef k;
    int fmt;

    YS_HD void load(int r, int c, int bgr[3]) const
    {
        if (!GENERAL) {
            const long long off = (long long)(r >> 1) * c_row + (long long)(c >> 1) * c_pix;
            yf_yuv_to_bgr(y[(long long)r * y_row + (long long)c * y_pix], u[off], v[off], k, bgr);
            return;
        }
        const unsigned char* py = y + (long long)r * y_row + (long long)c * y_pix;
        const long long off = (long long)(r >> ys_sy(fmt)) * c_row + (long long)(c >> ys_sx(fmt)) * c_pix;
        if (fmt & YS_16BIT) {
            int U = 32768, V = 32768;
            if (!(fmt & YS_GREY)) { U = ys_load16(u + off); V = ys_load16(v + off); }
            yf_yuv16_to_bgr(ys_load16(py), U, V, k, bgr);
        } else {
            int U = 128, V = 128;
            if (!(fmt & YS_GREY)) { U = u[off]; V = v[off]; }
            yf_yuv_to_bgr(*py, U, V, k, bgr);
        }
    }
};

// Desc: any mirror of cp_yuv_frame_desc
template <bool GENERAL, class Desc>
YS_HD YsSource<GENERAL> ys_source(const Desc& d, const YfCoef& k)
{
    YsSource<GENERAL> s = {d.y_base, d.u_base, d.v_base, d.y_row, d.y_pix, d.c_row, d.c_pix, k, d.pad};
    return s;
}

// the format word alone -> nullptr, or why it is refused
inline const char* ys_check_word(int fmt)
{
    if (fmt < 0 || fmt > YS_FORMAT_MAX) return "outside 0..15";
    if ((fmt & YS_GREY) && (fmt & (YS_FULL_X | YS_FULL_Y))) return "grey (bit 3) has no chroma for bits 0 / 1 to describe";
    return nullptr;
}

// What of one descriptor depends on its format -> nullptr, or why it is refused: the word itself, the bases it needs (a grey frame
// may have null chroma bases), strides >= 0, 2-byte alignment of every base and stride of 16-bit samples, and the last addressed
// offset of each plane below 2^62.  Sizes are the caller's to check first (H, W > 0).
template <class Desc>
inline const char* ys_check_format(const Desc& d)
{
    if (const char* why = ys_check_word(d.pad)) return why;
    const bool grey = (d.pad & YS_GREY) != 0;
    if (!d.y_base || (!grey && !(d.u_base && d.v_base))) return "null base address";
    if (d.y_row < 0 || d.y_pix < 0 || (!grey && (d.c_row < 0 || d.c_pix < 0))) return "negative stride";
    if (d.pad & YS_16BIT) {
        if (((size_t)d.y_base | (size_t)d.y_row | (size_t)d.y_pix) & 1) return "16-bit samples need even luma base and strides";
        if (!grey && (((size_t)d.u_base | (size_t)d.v_base | (size_t)d.c_row | (size_t)d.c_pix) & 1))
            return "16-bit samples need even chroma bases and strides";
    }
    const __int128 y_last = (__int128)(d.H - 1) * d.y_row + (__int128)(d.W - 1) * d.y_pix;
    const __int128 c_last = grey ? 0 : (__int128)((d.H - 1) >> ys_sy(d.pad)) * d.c_row + (__int128)((d.W - 1) >> ys_sx(d.pad)) * d.c_pix;
    if (y_last >= ((__int128)1 << 62) || c_last >= ((__int128)1 << 62)) return "strides address more than 2^62 bytes";
    return nullptr;
}
