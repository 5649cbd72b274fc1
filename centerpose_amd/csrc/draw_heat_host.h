// Host side of the heat-map overlay: the argument checks shared by the device launchers and the host painters, the scratch size, and the
// sequential host painters themselves (cp_draw_heat_frames_host / cp_draw_heat_yuv_frames_host, exported by draw_heat.hip).  Plain C++
// over draw_heat_arith.h, no device code and no HIP header: tools/draw_heat_host_fuzz.cpp compiles this file with the host compiler
// under AddressSanitizer / UBSan.  A failed check writes its message to `err` and returns 1.
//
// The host painters walk image by image, build the image's colour map, then every pixel (every 2 x 2 block) of the frame in raster
// order; the device does both steps as one launch each over all images.  The statements are those of draw_heat_arith.h either way.
#pragma once
#include <vector>
#include "draw_heat_arith.h"
#include "draw_host.h"

// scratch of one call: the colour maps, one dword per image and map cell
inline size_t dh_scratch_bytes(long long N, long long h, long long w)
{
    if (N <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)N * (size_t)h * (size_t)w * sizeof(uint32_t);
}

inline bool dh_finite(double v)
{
    union { double d; uint64_t u; } c;
    c.d = v;
    return ((c.u >> 52) & 0x7ffu) != 0x7ffu;
}

// what does not depend on the frames: N, the maps' shape and strides, the style, the matrix id (YUV).  *noop: N is 0, nothing else is
// looked at beyond the style.
inline int dh_check_call(const char* who, int N, const long long* stride, int C, int h, int w, const DhStyle* style, int matrix, bool* noop,
                         char* err, size_t errn)
{
    *noop = false;
    DR_CHECK(N >= 0 && N <= 65535, "%s: 0 to 65535 frames per call (got %d)", who, N);
    DR_CHECK(style, "%s: null style", who);
    DR_CHECK(C >= 1 && C <= DH_MAX_CHANNELS, "%s: %d map channels outside 1..%d", who, C, DH_MAX_CHANNELS);
    DR_CHECK(style->channels >= C && style->channels <= DH_MAX_CHANNELS, "%s: the style has %d colours for %d channels (%d..%d)", who,
             style->channels, C, C, DH_MAX_CHANNELS);
    DR_CHECK(style->opacity >= 1 && style->opacity <= DO_OPAQUE, "%s: opacity %d outside 1..%d", who, style->opacity, DO_OPAQUE);
    DR_CHECK(style->invert == 0 || style->invert == 1, "%s: invert is 0 or 1 (got %d)", who, style->invert);
    DR_CHECK(matrix == 0 || matrix == 1, "%s: matrix id %d is neither 0 (bt601) nor 1 (bt709)", who, matrix);
    DR_CHECK(h >= 1 && h <= DA_MAX_SIDE && w >= 1 && w <= DA_MAX_SIDE, "%s: bad map size %d x %d (1..%d)", who, h, w, DA_MAX_SIDE);
    DR_CHECK((long long)(N > 0 ? N : 1) * h * w <= DH_MAX_CELLS, "%s: %d maps of %d x %d cells are too many for one call", who, N, h, w);
    for (int i = 0; i < 4; ++i) {
        DR_CHECK(stride[i] >= 0, "%s: negative map stride %lld", who, stride[i]);
        DR_CHECK(stride[i] < (1ll << 40), "%s: map stride %lld is too large", who, stride[i]);
    }
    *noop = N == 0;
    return 0;
}

// the frame -> map matrix of every descriptor row (its `mi` field) is finite
template <class Desc>
inline int dh_check_matrices(const char* who, const Desc* t, int N, char* err, size_t errn)
{
    for (int n = 0; n < N; ++n)
        for (int i = 0; i < 6; ++i) DR_CHECK(dh_finite(t[n].mi[i]), "%s: frame %d: entry %d of the frame -> map matrix is not finite", who, n, i);
    return 0;
}

// HOST painter over cp_frame_desc (YUV = false) or cp_yuv_frame_desc (true) descriptors with host addresses and HOST maps
template <bool YUV>
inline int dh_draw_frames_host(const typename DrDesc<YUV>::type* table, int N, const float* maps, const long long* stride, int C, int h, int w,
                               const DhStyle* style, int matrix, char* err, size_t errn)
{
    const char* who = YUV ? "draw_heat_yuv_frames_host" : "draw_heat_frames_host";
    bool noop;
    if (int rc = dh_check_call(who, N, stride, C, h, w, style, matrix, &noop, err, errn)) return rc;
    if (noop) return 0;
    DR_CHECK(table && maps, "%s: null pointer", who);
    if constexpr (YUV) {
        if (int rc = dr_check_yuv_frames(who, table, N, err, errn)) return rc;
    } else {
        if (int rc = dr_check_frames(who, table, N, err, errn)) return rc;
    }
    if (int rc = dh_check_matrices(who, table, N, err, errn)) return rc;
    const int a = style->opacity;
    std::vector<uint32_t> cm((size_t)h * w);
    for (int n = 0; n < N; ++n) {
        const auto& d = table[n];
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j)
                cm[(size_t)i * w + j] = dh_cell(maps + n * stride[0] + i * stride[2] + j * stride[3], stride[1], C, *style);
        if constexpr (YUV) {
            for (int py = 0; py < d.H; py += 2)
                for (int px = 0; px < d.W; px += 2) {
                    int luma[4], uv[2];
                    dh_block_yuv(cm.data(), h, w, d.mi, px, py, d.H, d.W, matrix, luma, uv);
                    for (int q = 0; q < 4; ++q) {
                        const int x = px + (q & 1), y = py + (q >> 1);
                        if (x >= d.W || y >= d.H) continue;
                        unsigned char* p = d.y_base + (long long)y * d.y_row + (long long)x * d.y_pix;
                        *p = (unsigned char)do_blend(*p, luma[q], a);
                    }
                    const long long o = (long long)(py >> 1) * d.c_row + (long long)(px >> 1) * d.c_pix;
                    d.u_base[o] = (unsigned char)do_blend(d.u_base[o], uv[0], a);
                    d.v_base[o] = (unsigned char)do_blend(d.v_base[o], uv[1], a);
                }
        } else {
            for (int y = 0; y < d.H; ++y)
                for (int x = 0; x < d.W; ++x) {
                    int c[3];
                    dh_sample(cm.data(), h, w, d.mi, x, y, c);
                    unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
                    for (int k = 0; k < 3; ++k) p[d.ch_off[k]] = (unsigned char)do_blend(p[d.ch_off[k]], c[k], a);
                }
        }
    }
    return 0;
}
