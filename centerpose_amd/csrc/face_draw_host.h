// Host side of the face overlays: the argument checks shared by the device launchers and the host painters, and the sequential host
// painters themselves (cp_face_draw_frames_host / cp_face_draw_yuv_frames_host, exported by face_draw.hip).  Plain C++ over
// face_draw_arith.h and the descriptor mirrors and frame checks of draw_host.h, no device code and no HIP header.  A failed check
// writes its message to `err` and returns 1.  The host painters paint forward -- the vertices of all faces, then the faces in
// ascending slot order, primitives in paint order, a later store over an earlier one -- where the device looks for the last covering
// primitive from the back.
#pragma once
#include "draw_host.h"
#include "face_draw_arith.h"

inline size_t fd_scratch_bytes(int cap)
{
    if (cap < 1 || cap > FD_MAX_CAP) return 0;
    return (size_t)cap * (sizeof(FdHeader) + FD_STRIDE * sizeof(DaPrim));
}

// what a call is given beside the frames (all DEVICE pointers for the launchers, HOST pointers for the host painters)
struct FdFaces {
    const int* slots;            // [cap]
    const float* landmarks;      // [cap, 68, 3]
    const int* box;              // [cap, 10, 2] or null
    const int* valid;            // [cap] or null
    const float* pos;            // [cap, 256, 256, 3] or null
    const int* face_ind;         // [V] or null
    int V;
};

inline int fd_check_call(const char* who, int N, int cap, const FdFaces& f, const FdStyle* st, char* err, size_t errn)
{
    DR_CHECK(cap >= 1 && cap <= FD_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FD_MAX_CAP);
    DR_CHECK(N >= 1 && N <= cap, "%s: %d frames for a capacity of %d", who, N, cap);
    DR_CHECK(st, "%s: null style", who);
    const int radii[4] = {st->landmark_radius, st->line_radius, st->box_radius, st->vertex_radius};
    for (int i = 0; i < 4; ++i) DR_CHECK(radii[i] >= 0 && radii[i] <= FD_MAX_RADIUS, "%s: radius %d outside 0..%d", who, radii[i], FD_MAX_RADIUS);
    DR_CHECK(st->vertex_step >= 1, "%s: vertex_step %d below 1", who, st->vertex_step);
    DR_CHECK(f.slots && f.landmarks, "%s: null pointer", who);
    DR_CHECK(!st->pose_box || (f.box && f.valid), "%s: pose_box without a pose (null box or valid)", who);
    DR_CHECK(!st->vertices || (f.pos && f.face_ind), "%s: vertices without position maps or face_ind", who);
    DR_CHECK(!st->vertices || (f.V >= 1 && f.V <= FD_CELLS), "%s: %d vertices outside 1..%d", who, f.V, FD_CELLS);
    return 0;
}

// The pixels of one face in paint order: put(x, y, colour class)
template <class Put>
inline void fd_paint_face(const FdFaces& f, int s, const FdStyle& st, int H, int W, Put put)
{
    for (int i = 0; i < FD_PRIMS; ++i) {
        DaPrim p;
        if (!fd_build(f.landmarks + (size_t)s * FD_NKPT * 3, f.box ? f.box + (size_t)s * 20 : nullptr, f.valid ? f.valid[s] : 0, st, i, &p))
            continue;
        int x0, y0, x1, y1;
        da_bounds(p, fd_radius(st, i), &x0, &y0, &x1, &y1);
        if (x0 < 0) x0 = 0;
        if (y0 < 0) y0 = 0;
        if (x1 > W - 1) x1 = W - 1;
        if (y1 > H - 1) y1 = H - 1;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x)
                if (fd_covers(p, i, st, x, y)) put(x, y, fd_class(i));
    }
}

// The dense vertices of one face: put(x, y, 2)
template <class Put>
inline void fd_paint_vertices(const FdFaces& f, int s, const FdStyle& st, int H, int W, Put put)
{
    const int R = st.vertex_radius, count = fd_vertex_count(f.V, st.vertex_step);
    const long long k = (long long)R * R + R;
    for (int j = 0; j < count; ++j) {
        int cx, cy;
        if (!fd_vertex(f.pos + (size_t)s * FD_CELLS * 3, f.face_ind, f.V, st, j, &cx, &cy)) continue;
        for (int y = cy - R; y <= cy + R; ++y)
            for (int x = cx - R; x <= cx + R; ++x)
                if (x >= 0 && x < W && y >= 0 && y < H && da_disc(x - cx, y - cy, k)) put(x, y, 2);
    }
}

template <class Desc, class Put>
inline void fd_paint_frames(const Desc* table, int N, int cap, const FdFaces& f, const FdStyle& st, Put put)
{
    const int q = cap / N;
    for (int n = 0; n < N; ++n) {
        const Desc& d = table[n];
        if (st.vertices)
            for (int s = n * q; s < n * q + q; ++s)
                if (f.slots[s] >= 0) fd_paint_vertices(f, s, st, d.H, d.W, [&](int x, int y, int c) { put(d, x, y, c); });
        for (int s = n * q; s < n * q + q; ++s)
            if (f.slots[s] >= 0) fd_paint_face(f, s, st, d.H, d.W, [&](int x, int y, int c) { put(d, x, y, c); });
    }
}

// HOST painter over cp_frame_desc descriptors with host addresses; style colours are in the frame's channel order of (B, G, R)
inline int fd_draw_frames_host(const DrFrameDesc* table, int N, int cap, const FdFaces& f, const FdStyle* st, char* err, size_t errn)
{
    const char* who = "face_draw_frames_host";
    if (int rc = fd_check_call(who, N, cap, f, st, err, errn)) return rc;
    DR_CHECK(table, "%s: null pointer", who);
    if (int rc = dr_check_frames(who, table, N, err, errn)) return rc;
    fd_paint_frames(table, N, cap, f, *st, [&](const DrFrameDesc& d, int x, int y, int c) {
        unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
        for (int k = 0; k < 3; ++k) p[d.ch_off[k]] = st->colors[c][k];
    });
    return 0;
}

// HOST painter over cp_yuv_frame_desc descriptors; style colours are (Y, U, V).  Every covered pixel stores its luma and the chroma
// sample of its 2x2 block, so the sample ends with the colour of the last primitive that covers any of the four.
inline int fd_draw_yuv_frames_host(const DrYuvFrameDesc* table, int N, int cap, const FdFaces& f, const FdStyle* st, char* err, size_t errn)
{
    const char* who = "face_draw_yuv_frames_host";
    if (int rc = fd_check_call(who, N, cap, f, st, err, errn)) return rc;
    DR_CHECK(table, "%s: null pointer", who);
    if (int rc = dr_check_yuv_frames(who, table, N, err, errn)) return rc;
    fd_paint_frames(table, N, cap, f, *st, [&](const DrYuvFrameDesc& d, int x, int y, int c) {
        const long long ci = (long long)(y >> 1) * d.c_row + (long long)(x >> 1) * d.c_pix;
        d.y_base[(long long)y * d.y_row + (long long)x * d.y_pix] = st->colors[c][0];
        d.u_base[ci] = st->colors[c][1];
        d.v_base[ci] = st->colors[c][2];
    });
    return 0;
}
