// The rule of the 3-D face stage, once, for the host and the device: which candidates get a face crop, the similarity that cuts the
// 256 x 256 network input out of the frame, the value of every pixel of that input, and the way the network's position map goes back
// to image coordinates.  face_stage.hip compiles these statements into its kernels, face_host.h into the sequential host twins (what a
// test pins).  float32 throughout; include from a translation unit compiled with -ffp-contract=off: one rounding per operation.
//
// This restates PRN.process of the reference's video demo (demo/face/prnet.py:83-117) in closed form.  The reference estimates the
// similarity with skimage (estimate_transform) and samples with skimage's warp; neither is available to this project, so the rule
// below is a statement of that pipeline, NOT pinned to a recording of it.
//
// Box (prnet.py:83-93): a candidate gives (left, right, top, bottom) -- the min / max of its five face joints (nose, eyes, ears:
// floats 5..14 of a detection row, x and y interleaved) or a given box (x1, y1, x2, y2, score) read as left = x1, right = x2, top = y1,
// bottom = y2.  old_size = ((right - left) + bottom - top) / 2, size = (int)(old_size * expand), centre cx = right - (right - left) / 2,
// cy = bottom - (bottom - top) / 2.  A candidate is selected iff its score is > vis_thresh (strict; a NaN score is not), every
// coordinate it reads is finite and min_size <= size <= 32768.  The crop is the square of side `size` around the centre:
// x0 = cx - size / 2, y0 = cy - size / 2.
//
// Crop (prnet.py:97-102; warp(image / 255., tform.inverse, (256, 256)) with skimage's defaults: order 1, mode 'constant', cval 0):
// output pixel (u, v) samples the frame at x = x0 + u * (size / 255), y = y0 + v * (size / 255); ix = floor(x), a = x - ix, likewise
// iy, b; the four neighbours (ix, iy) .. (ix + 1, iy + 1) are blended horizontally, then vertically, with the weights (1 - a, a) and
// (1 - b, b); a neighbour outside the frame contributes 0; the result is divided by 255.  Channels are written in R, G, B order.
//
// Restore (prnet.py:106-115): P = out * 256 * 1.1 (the float32 product 281.6); x = P_x * (size / 255) + x0, y likewise,
// z = P_z * (size / 255).  Landmark k is the restored cell (row uv[1][k], column uv[0][k]) of the map (get_landmarks, :119-127).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FA_HD __host__ __device__ inline
#else
#define FA_HD inline
#endif

#define FA_ROW 56            // floats per detection row
#define FA_BOX 5             // floats per given box
#define FA_RES 256           // the network's input and output resolution
#define FA_NKPT 68           // landmarks
#define FA_MAX_SIZE 32768
#define FA_MAX_CAP 256
#define FA_MAX_ROWS (1 << 24)        // N * M: a slot entry n * M + m fits an int with room

struct FaXform { float x0, y0, size; };     // a slot's similarity: frame x = x0 + u * size / 255

FA_HD bool fa_finite(float v) { return v - v == 0.f; }

// (left, right, top, bottom) -> the crop square; false: not selected
FA_HD bool fa_square(float left, float right, float top, float bottom, float expand, int min_size, FaXform* t)
{
    if (!(fa_finite(left) && fa_finite(right) && fa_finite(top) && fa_finite(bottom))) return false;
    const float w = right - left, h = bottom - top;
    const float old_size = ((w + bottom) - top) / 2.f;
    const float fs = old_size * expand;
    if (!(fs >= (float)min_size && fs < (float)(FA_MAX_SIZE + 1))) return false;     // (int)fs in min_size..32768; NaN fails
    const int size = (int)fs;
    const float cx = right - w / 2.f, cy = bottom - h / 2.f;
    const float half = (float)size / 2.f;
    t->x0 = cx - half;
    t->y0 = cy - half;
    t->size = (float)size;
    return true;
}

// a detection row: the five face joints
FA_HD bool fa_select_row(const float* row, float vis_thresh, float expand, int min_size, FaXform* t)
{
    if (!(row[4] > vis_thresh)) return false;
    float left = row[5], right = row[5], top = row[6], bottom = row[6];
    bool finite = true;
    for (int j = 0; j < 5; ++j) {
        const float x = row[5 + 2 * j], y = row[6 + 2 * j];
        finite = finite && fa_finite(x) && fa_finite(y);
        left = x < left ? x : left;
        right = x > right ? x : right;
        top = y < top ? y : top;
        bottom = y > bottom ? y : bottom;
    }
    return finite && fa_square(left, right, top, bottom, expand, min_size, t);
}

// a given box (x1, y1, x2, y2, score)
FA_HD bool fa_select_box(const float* box, float vis_thresh, float expand, int min_size, FaXform* t)
{
    if (!(box[4] > vis_thresh)) return false;
    return fa_square(box[0], box[2], box[1], box[3], expand, min_size, t);
}

FA_HD bool fa_select(const float* cand, int boxes, float vis_thresh, float expand, int min_size, FaXform* t)
{
    return boxes ? fa_select_box(cand, vis_thresh, expand, min_size, t) : fa_select_row(cand, vis_thresh, expand, min_size, t);
}

FA_HD float fa_step(float size) { return size / 255.f; }

// One axis of one output pixel: the first neighbour, whether each neighbour lies inside 0..n-1, and the weight of the second.
// A coordinate that is not finite or lies a pixel or more outside the frame has no neighbour inside.
struct FaTap { int i; bool in0, in1; float f; };

FA_HD FaTap fa_tap(float origin, float step, int o, int n)
{
    const float x = origin + (float)o * step;
    FaTap t = {0, false, false, 0.f};
    if (!(x > -1.f && x < (float)n)) return t;
    const float fl = floorf(x);
    t.i = (int)fl;
    t.f = x - fl;
    t.in0 = t.i >= 0;
    t.in1 = t.i + 1 < n;
    return t;
}

FA_HD float fa_blend(float p00, float p01, float p10, float p11, float a, float b)
{
    const float top = p00 * (1.f - a) + p01 * a;
    const float bot = p10 * (1.f - a) + p11 * a;
    return (top * (1.f - b) + bot * b) / 255.f;
}

// One output pixel (u = column, v = row) of the crop `t` of an H x W frame: src.load(y, x, p) puts the frame's (B, G, R) of pixel
// (y, x) into p[0..2]; r = (R, G, B).
template <class Src>
FA_HD void fa_pixel(const Src& src, int H, int W, const FaXform& t, int v, int u, float r[3])
{
    const float step = fa_step(t.size);
    const FaTap tx = fa_tap(t.x0, step, u, W), ty = fa_tap(t.y0, step, v, H);
    int p[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (ty.in0 && tx.in0) src.load(ty.i, tx.i, p[0]);
    if (ty.in0 && tx.in1) src.load(ty.i, tx.i + 1, p[1]);
    if (ty.in1 && tx.in0) src.load(ty.i + 1, tx.i, p[2]);
    if (ty.in1 && tx.in1) src.load(ty.i + 1, tx.i + 1, p[3]);
    for (int k = 0; k < 3; ++k)
        r[k] = fa_blend((float)p[0][2 - k], (float)p[1][2 - k], (float)p[2][2 - k], (float)p[3][2 - k], tx.f, ty.f);
}

// One cell (three network outputs in 0..1) back to image coordinates
FA_HD void fa_restore(const FaXform& t, float ox, float oy, float oz, float r[3])
{
    const float gain = 256.f * 1.1f, step = fa_step(t.size);
    r[0] = (ox * gain) * step + t.x0;
    r[1] = (oy * gain) * step + t.y0;
    r[2] = (oz * gain) * step;
}
