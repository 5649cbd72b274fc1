// Host side of the mesh rasteriser: the argument checks shared by the device launchers and the host twins, and the sequential host
// twins themselves (cp_face_render_host / cp_face_vertex_colors_host / cp_face_vertex_colors_yuv_host, exported by face_render.hip).
// Plain C++ over face_render_arith.h and the descriptor mirrors, samplers and frame checks of reid_host.h, no device code and no HIP
// header: tools/face_render_host_fuzz.cpp compiles this file with the host compiler under AddressSanitizer / UBSan.  A failed check
// writes its message to `err` and returns 1.
#pragma once
#include "face_render_arith.h"
#include "reid_host.h"

// the key buffer: one 64-bit key per pixel of every slot's window
inline size_t fr_scratch_bytes(int cap, int h, int w) { return (size_t)cap * h * w * sizeof(uint64_t); }

inline int fr_check_sizes(const char* who, int cap, int V, int T, int h, int w, char* err, size_t errn)
{
    RH_CHECK(cap >= 1 && cap <= FR_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FR_MAX_CAP);
    RH_CHECK(V >= FR_MIN_V && V <= FR_MAX_V, "%s: %d vertices outside %d..%d", who, V, FR_MIN_V, FR_MAX_V);
    RH_CHECK(T >= 1 && T <= FR_MAX_T, "%s: %d triangles outside 1..%d", who, T, FR_MAX_T);
    RH_CHECK(h >= 1 && h <= FR_MAX_SIDE && w >= 1 && w <= FR_MAX_SIDE, "%s: window %d x %d outside 1..%d", who, h, w, FR_MAX_SIDE);
    RH_CHECK((long long)cap * h * w * 8 < (1ll << 31), "%s: %d windows of %d x %d: the key buffer reaches 2^31 bytes", who, cap, h, w);
    return 0;
}

inline int fr_check_call(const char* who, int cap, int V, int T, int h, int w, int C, bool attrs, size_t scratch_bytes, char* err, size_t errn)
{
    if (int rc = fr_check_sizes(who, cap, V, T, h, w, err, errn)) return rc;
    RH_CHECK(C >= 1 && C <= FR_MAX_C, "%s: %d attribute channels outside 1..%d", who, C, FR_MAX_C);
    RH_CHECK(attrs || C == 1, "%s: no attributes (the vertices' z) with %d channels: one", who, C);
    RH_CHECK(scratch_bytes >= fr_scratch_bytes(cap, h, w), "%s: %zu bytes of scratch, %zu needed (cp_face_render_scratch_bytes)", who,
             scratch_bytes, fr_scratch_bytes(cap, h, w));
    return 0;
}

inline int fr_check_face_ind(const char* who, const int* face_ind, int V, char* err, size_t errn)
{
    for (int k = 0; k < V; ++k) RH_CHECK(face_ind[k] >= 0 && face_ind[k] < FR_CELLS, "%s: face_ind[%d] = %d outside the map", who, k, face_ind[k]);
    return 0;
}

// HOST render: pos [cap, 256, 256, 3], slots [cap] and origin [cap, 2] (fr_slot_used), face_ind [V], tri [T, 3],
// attrs [cap, V, C] or null (z) -> scratch (the keys [cap, h, w]), out_tri [cap, h, w], out_image [cap, h, w, C].  The twin also checks
// the two tables, which the device launcher leaves to the caller.
inline int fr_render_host(const float* pos, const int* slots, int cap, const int* face_ind, int V, const int* tri, int T, const int* origin,
                          int h, int w, const float* attrs, int C, uint64_t* scratch, size_t scratch_bytes, int* out_tri, float* out_image,
                          char* err, size_t errn)
{
    const char* who = "face_render_host";
    if (int rc = fr_check_call(who, cap, V, T, h, w, C, attrs != nullptr, scratch_bytes, err, errn)) return rc;
    RH_CHECK(pos && slots && face_ind && tri && origin && scratch && out_tri && out_image, "%s: null pointer", who);
    if (int rc = fr_check_face_ind(who, face_ind, V, err, errn)) return rc;
    for (size_t k = 0; k < (size_t)3 * T; ++k)
        RH_CHECK(tri[k] >= 0 && tri[k] < V, "%s: triangle %zu names vertex %d of %d", who, k / 3, tri[k], V);
    const size_t window = (size_t)h * w;
    for (size_t k = 0; k < cap * window; ++k) scratch[k] = 0;
    for (int s = 0; s < cap; ++s) {
        if (!fr_slot_used(slots, origin, s)) continue;
        const float* map = pos + (size_t)s * FR_CELLS * 3;
        uint64_t* keys = scratch + s * window;
        const int x0 = origin[2 * s], y0 = origin[2 * s + 1];
        for (int i = 0; i < T; ++i) {
            const float* p[3];
            fr_gather(map, face_ind, tri, i, p);
            FrTri t;
            if (!fr_setup(p[0], p[1], p[2], x0, y0, h, w, &t)) continue;
            const uint64_t key = fr_key(t.d, i);
            for (int Y = t.vmin; Y <= t.vmax; ++Y)
                for (int X = t.umin; X <= t.umax; ++X) {
                    uint64_t* k = keys + (size_t)(Y - y0) * w + (X - x0);
                    if (fr_covers(t, X, Y) && key > *k) *k = key;
                }
        }
    }
    for (int s = 0; s < cap; ++s) {
        const float* map = pos + (size_t)s * FR_CELLS * 3;
        for (size_t px = 0; px < window; ++px) {
            const size_t o = s * window + px;
            fr_resolve(scratch[o], map, face_ind, tri, attrs ? attrs + (size_t)s * V * C : nullptr, C, out_tri + o, out_image + o * C);
        }
    }
    return 0;
}

inline int fr_check_colors(const char* who, int N, int cap, int V, char* err, size_t errn)
{
    RH_CHECK(cap >= 1 && cap <= FR_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FR_MAX_CAP);
    RH_CHECK(N >= 1 && N <= cap, "%s: %d frames for a capacity of %d", who, N, cap);
    RH_CHECK(V >= FR_MIN_V && V <= FR_MAX_V, "%s: %d vertices outside %d..%d", who, V, FR_MIN_V, FR_MAX_V);
    return 0;
}

// HOST vertex colours: frame n owns slots n * q .. n * q + q - 1, q = cap / N -> colors [cap, V, 3] = (B, G, R), zeros for a slot that is
// unused or beyond N * q
template <class Desc, class Make>
inline void fr_colors(const Desc* table, int N, const float* pos, const int* slots, int cap, const int* face_ind, int V, float* colors,
                      Make make)
{
    const int q = cap / N;
    for (int s = 0; s < cap; ++s) {
        float* o = colors + (size_t)s * V * 3;
        if (slots[s] < 0 || s / q >= N) {
            for (size_t k = 0; k < (size_t)V * 3; ++k) o[k] = 0.f;
            continue;
        }
        const Desc& d = table[s / q];
        const auto src = make(d);
        for (int k = 0; k < V; ++k) fr_color(src, d.H, d.W, pos + ((size_t)s * FR_CELLS + face_ind[k]) * 3, o + (size_t)k * 3);
    }
}

inline int fr_colors_host(const RhFrameDesc* table, int N, const float* pos, const int* slots, int cap, const int* face_ind, int V,
                          float* colors, char* err, size_t errn)
{
    const char* who = "face_vertex_colors_host";
    if (int rc = fr_check_colors(who, N, cap, V, err, errn)) return rc;
    RH_CHECK(table && pos && slots && face_ind && colors, "%s: null pointer", who);
    if (int rc = rh_check_frames(who, table, N, err, errn)) return rc;
    if (int rc = fr_check_face_ind(who, face_ind, V, err, errn)) return rc;
    fr_colors(table, N, pos, slots, cap, face_ind, V, colors, [](const RhFrameDesc& d) { return rh_source(d); });
    return 0;
}

inline int fr_colors_yuv_host(const RhYuvFrameDesc* table, int N, const int* coef, const float* pos, const int* slots, int cap,
                              const int* face_ind, int V, float* colors, char* err, size_t errn)
{
    const char* who = "face_vertex_colors_yuv_host";
    if (int rc = fr_check_colors(who, N, cap, V, err, errn)) return rc;
    RH_CHECK(table && pos && slots && face_ind && colors, "%s: null pointer", who);
    if (int rc = rh_check_yuv_frames(who, table, N, coef, err, errn)) return rc;
    if (int rc = fr_check_face_ind(who, face_ind, V, err, errn)) return rc;
    const YfCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    fr_colors(table, N, pos, slots, cap, face_ind, V, colors, [&](const RhYuvFrameDesc& d) { return rh_yuv_source<true>(d, k); });
    return 0;
}
