// The drawing rule of the face overlays, once, for the host and the device: which primitives a face has and which pixels each covers.
// face_draw.hip compiles these statements into its kernels, face_draw_host.h into the sequential host painters (what a test pins).
// The picture is this project's rule, not cv2's rasteriser: the disc and capsule statements of draw_arith.h (k = R^2 + R, a squared
// cross product, all products in 64 bits); the content is the reference's plot_kpt, plot_vertices and plot_pose_box
// (demo/face/utils/cv_plot.py).
//
// A landmark or vertex sits at rint (half to even, np.round) of its float32 x and y, clamped to [-16384, 16384] first; a coordinate
// that is not finite kills the primitives it belongs to.  The 141 primitives of a face in paint order:
//   0..59    capsules k -> k + 1 of radius line_radius for every landmark k not in end_list (cv_plot.py:9: 16, 21, 26, 30, 35, 41, 47, 67)
//   60..127  a disc of radius landmark_radius on every landmark
//   128..140 the pose box, capsules of radius box_radius: the closed polyline over the ten corners, then 1 -> 6, 2 -> 7, 3 -> 8; only
//            with style.pose_box and where the pose is valid
// style.landmarks switches 0..127.  Faces are painted in ascending slot order (frame n owns slots n * q .. n * q + q - 1, q = cap / N;
// a slot is used iff slots[s] >= 0), the last painter wins, stores are opaque, everything is clipped.  Beneath all faces of a frame lie
// the dense vertices (style.vertices): a disc of radius vertex_radius at vertex i * vertex_step of face_ind, i = 0, 1, ...; every such
// store writes the same bytes, so their order does not matter.
#pragma once
#include <math.h>
#include "draw_arith.h"

#define FD_SEGS 60
#define FD_DISCS 68
#define FD_BOXSEGS 13
#define FD_PRIMS (FD_SEGS + FD_DISCS + FD_BOXSEGS)      // 141
#define FD_STRIDE 144                                    // primitive records per face in the scratch
#define FD_MAX_RADIUS 3
#define FD_MAX_CAP 256
#define FD_NKPT 68
#define FD_CELLS 65536

// mirror of cp_face_style (include/centerpose_hip.h); colours: landmark, line, vertex, box -- bytes 0..2 are what is stored
struct FdStyle {
    int landmarks, vertices, pose_box;
    int landmark_radius, line_radius, box_radius, vertex_radius, vertex_step;
    unsigned char colors[4][4];
};
static_assert(sizeof(FdStyle) == 48, "cp_face_style is 48 bytes");

// per face in the scratch: the bounding box of what it can cover and the mask of its existing primitives
struct FdHeader { int x0, y0, x1, y1; unsigned long long mask[3]; unsigned long long pad; };
static_assert(sizeof(FdHeader) == 48, "face header is 48 bytes");

DA_HD bool fd_coord(float v, int* out)
{
    if (!da_finite(v)) return false;
    const float c = v < -16384.f ? -16384.f : (v > 16384.f ? 16384.f : v);
    *out = (int)rintf(c);
    return true;
}

DA_HD bool fd_point(const float* xyz, int* x, int* y)
{
    const bool a = fd_coord(xyz[0], x), b = fd_coord(xyz[1], y);
    return a && b;
}

// the first landmark of segment i
DA_HD int fd_seg_start(int i)
{
    constexpr unsigned char K[FD_SEGS] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 17, 18, 19, 20,
                                          22, 23, 24, 25, 27, 28, 29, 31, 32, 33, 34, 36, 37, 38, 39, 40, 42, 43, 44, 45,
                                          46, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 66};
    return K[i];
}

DA_HD int fd_class(int i) { return i < FD_SEGS ? 1 : (i < FD_SEGS + FD_DISCS ? 0 : 3); }       // index into style.colors
DA_HD int fd_radius(const FdStyle& st, int i) { return i < FD_SEGS ? st.line_radius : (i < FD_SEGS + FD_DISCS ? st.landmark_radius : st.box_radius); }

// primitive i of a used face: landmarks [68, 3] of the slot, box [10, 2] and valid of its pose (box may be null) -> whether it exists
DA_HD bool fd_build(const float* landmarks, const int* box, int valid, const FdStyle& st, int i, DaPrim* p)
{
    if (i < FD_SEGS) {
        if (!st.landmarks) return false;
        const int k = fd_seg_start(i);
        const bool a = fd_point(landmarks + 3 * k, &p->x0, &p->y0), b = fd_point(landmarks + 3 * (k + 1), &p->x1, &p->y1);
        return a && b;
    }
    if (i < FD_SEGS + FD_DISCS) {
        if (!st.landmarks) return false;
        const bool a = fd_point(landmarks + 3 * (i - FD_SEGS), &p->x0, &p->y0);
        p->x1 = p->x0; p->y1 = p->y0;
        return a;
    }
    if (!st.pose_box || !box || valid != 1) return false;
    const int j = i - FD_SEGS - FD_DISCS;
    const int a = j < 10 ? j : j - 9, b = j < 10 ? (j + 1) % 10 : j - 4;          // 10: 1 -> 6, 11: 2 -> 7, 12: 3 -> 8
    p->x0 = box[2 * a]; p->y0 = box[2 * a + 1]; p->x1 = box[2 * b]; p->y1 = box[2 * b + 1];
    return true;
}

// whether primitive p of index i covers pixel (x, y): da_covers' capsule (its limb) or disc (its joint) with the class's radius
DA_HD bool fd_covers(const DaPrim& p, int i, const FdStyle& st, int x, int y)
{
    const int R = fd_radius(st, i);
    const bool disc = i >= FD_SEGS && i < FD_SEGS + FD_DISCS;
    return da_covers(p, disc ? DA_PRIMS - 1 : 1, 0, R, R, x, y);
}

// the last primitive of one face that covers (x, y), from the back; -1: none
DA_HD int fd_face_winner(const DaPrim* prims, const FdHeader& h, const FdStyle& st, int x, int y)
{
    if (x < h.x0 || x > h.x1 || y < h.y0 || y > h.y1) return -1;
    for (int i = FD_PRIMS - 1; i >= 0; --i)
        if (((h.mask[i >> 6] >> (i & 63)) & 1) && fd_covers(prims[i], i, st, x, y)) return i;
    return -1;
}

// dense vertex j of a face (vertex j * vertex_step of face_ind) from its restored map pos [256, 256, 3] -> its pixel; false: not drawn
DA_HD bool fd_vertex(const float* pos, const int* face_ind, int V, const FdStyle& st, int j, int* x, int* y)
{
    const long long v = (long long)j * st.vertex_step;
    if (v >= V) return false;
    const int cell = face_ind[v];
    if (cell < 0 || cell >= FD_CELLS) return false;
    return fd_point(pos + 3 * (size_t)cell, x, y);
}

DA_HD int fd_vertex_count(int V, int step) { return (V + step - 1) / step; }
