// The rule of the head-pose stage, once, for the host and the device: the similarity that takes the canonical face cloud onto a slot's
// vertices, its Euler angles and the ten corners of the pose box.  face_pose.hip compiles these statements into its kernels,
// face_pose_host.h into the sequential host twin (what a test pins).  float64 throughout, only + - * / sqrt up to the angles; include
// from a translation unit compiled with -ffp-contract=off: one rounding per operation, so the device and the host give the same bits.
//
// This restates estimate_pose of the reference's video demo (demo/face/utils/estimate_pose.py:67-99) and the corners of plot_pose_box
// (demo/face/utils/cv_plot.py:48-70):
//
//   p0: the slot's V vertices, cell face_ind[v] of its restored position map -- the float32 values fa_restore gives (face_arith.h),
//       taken as float64.  p1: the canonical cloud; the host centres it once (q = p1 - m1) and gives q, m1 and rms_d1.
//   moments: with the pivot c = p0[0] (a vertex of the cloud itself, so nothing below cancels by more than the cloud's own extent over
//       its spread, wherever the face lies in the frame, and V identical vertices give exact zeros) and d = p0 - c:
//       S1 = sum d, C = sum d q^T, S2 = sum |d|^2 -- 13 sums, in the fixed order below.
//   m0 = c + S1 / V;  cov = C (sum (p0 - m0) q^T differs from it by (m0 - c)(sum q)^T, and q sums to zero up to its rounding);
//   rms_d0 = sqrt((S2 - |S1|^2 / V) / V).
//   U S W^T = svd(cov), R = U W^T: the orthogonal polar factor of cov, here by a cyclic one-sided Jacobi (fp_polar); if det R < 0,
//   column 2 of R is negated (the reference's own fix, kept).  s = rms_d0 / rms_d1, P = [s R | m0 - m1].
//   angles: P2sRt -- r1, r2 the normalised first two rows of P, r3 = r1 x r2 -- then matrix2angle: x = asin(r3[0]) (clamped to -1..1;
//       the reference raises beyond), y = atan2(r3[1] / cos x, r3[2] / cos x), z = atan2(r2[0] / cos x, r1[0] / cos x).  The Gimbal
//       branch of the reference (:29) is dead code and is not restated.
//   box: the corners (+-90, +-90, 0) and (+-105, +-105, 110) in the reference's order; [X, Y, Z, 1] . P^T[:, :2], minus the mean of the
//       first four, plus the mean of landmarks 0..26 (float32 values as float64, added in ascending order); clamped to -16384..16383
//       and truncated toward zero (a coordinate that is not a number gives 0).
//   valid = every one of the 13 moments is finite (one vertex that is not makes S2 infinite or NaN) and rms_d0 > 0 and rms_d1 > 0;
//       otherwise every output of the slot is zero.
//
// Summation order: vertex v belongs to chunk v / 2048; in a chunk lane l of 256 starts from 0 and adds v = base + l, base + l + 256, ...
// in ascending order (a lane beyond V adds nothing); the 256 lanes are combined by a binary tree over the lane index (stride 128 .. 1:
// lane l += lane l + stride); chunks are added in ascending order starting from 0.  No floating-point atomics.
#pragma once
#include <math.h>
#include <stdint.h>
#include "face_arith.h"

#define FP_CHUNK 2048          // vertices per chunk
#define FP_LANES 256           // lanes per chunk
#define FP_NMOM 13             // S1[3], C[3][3] (row: p0's axis), S2
#define FP_MIN_V 3
#define FP_MAX_V 65536
#define FP_CELLS (FA_RES * FA_RES)
#define FP_NBOX 10
#define FP_SWEEPS 30

struct FpPose { double P[12], angles[3], scale; int box[2 * FP_NBOX], valid; };

FA_HD int fp_chunks(int V) { return (V + FP_CHUNK - 1) / FP_CHUNK; }
// doubles of scratch per slot: the chunks' partial moments, then the pivot
FA_HD size_t fp_slot_doubles(int V) { return (size_t)fp_chunks(V) * FP_NMOM + 3; }
FA_HD bool fp_finite(double v) { return v - v == 0.0; }

// One vertex of a slot as float64.  NET: src is the plan's output [3, 256, 256] of the slot, restored on the fly; otherwise its
// restored map [256, 256, 3].  A cell outside the map gives a vertex that is not a number: the slot becomes invalid.
template <bool NET>
FA_HD void fp_vertex(const float* src, const FaXform& t, int cell, double p[3])
{
    if (cell < 0 || cell >= FP_CELLS) {
        p[0] = p[1] = p[2] = (double)NAN;
        return;
    }
    float r[3];
    if (NET) {
        fa_restore(t, src[cell], src[FP_CELLS + cell], src[2 * FP_CELLS + cell], r);
    } else {
        r[0] = src[3 * (size_t)cell]; r[1] = src[3 * (size_t)cell + 1]; r[2] = src[3 * (size_t)cell + 2];
    }
    p[0] = (double)r[0]; p[1] = (double)r[1]; p[2] = (double)r[2];
}

// acc += the moments' terms of one vertex p (pivot c) and its canonical partner q
FA_HD void fp_accumulate(double acc[FP_NMOM], const double p[3], const double c[3], const double q[3])
{
    double d[3];
    for (int i = 0; i < 3; ++i) d[i] = p[i] - c[i];
    for (int i = 0; i < 3; ++i) acc[i] += d[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) acc[3 + 3 * i + j] += d[i] * q[j];
    acc[12] += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

// What lane l of chunk `chunk` adds up
template <bool NET>
FA_HD void fp_lane(const float* src, const FaXform& t, const int* face_ind, int V, const double* canon, const double c[3], int chunk, int l,
                   double acc[FP_NMOM])
{
    for (int k = 0; k < FP_NMOM; ++k) acc[k] = 0.0;
    for (int i = 0; i < FP_CHUNK / FP_LANES; ++i) {
        const int v = chunk * FP_CHUNK + i * FP_LANES + l;
        if (v >= V) break;
        double p[3];
        fp_vertex<NET>(src, t, face_ind[v], p);
        fp_accumulate(acc, p, c, canon + 3 * (size_t)v);
    }
}

FA_HD double fp_norm3(const double* a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

FA_HD void fp_cross(const double* a, const double* b, double* r)
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// Column j of a row-major 3 x 3
#define FP_COL(m, j, v) do { (v)[0] = (m)[j]; (v)[1] = (m)[3 + j]; (v)[2] = (m)[6 + j]; } while (0)

// R = U W^T of A = U S W^T (row-major 3 x 3; A finite).  One-sided Jacobi: plane rotations from the right make A's columns orthogonal,
// B = A W; a column of B over its length is a column of U.  Columns that vanish (rank below three) are completed to a right-handed
// orthonormal basis: any completion is a polar factor of a singular matrix.
FA_HD void fp_polar(const double A[9], double R[9])
{
    double B[9], W[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double top = 0.0;
    for (int i = 0; i < 9; ++i) top = fabs(A[i]) > top ? fabs(A[i]) : top;
    for (int i = 0; i < 9; ++i) B[i] = top > 0.0 ? A[i] / top : 0.0;          // R does not depend on A's scale
    for (int sweep = 0; sweep < FP_SWEEPS; ++sweep) {
        bool turned = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double a[3], b[3];
                FP_COL(B, p, a);
                FP_COL(B, q, b);
                const double alpha = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], beta = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
                const double gamma = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
                if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) continue;
                turned = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tn = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
                for (int i = 0; i < 3; ++i) {
                    const double bp = B[3 * i + p], bq = B[3 * i + q], wp = W[3 * i + p], wq = W[3 * i + q];
                    B[3 * i + p] = cs * bp - sn * bq;
                    B[3 * i + q] = sn * bp + cs * bq;
                    W[3 * i + p] = cs * wp - sn * wq;
                    W[3 * i + q] = sn * wp + cs * wq;
                }
            }
        if (!turned) break;
    }
    double U[9], len[3], longest = 0.0;
    for (int j = 0; j < 3; ++j) {
        double a[3];
        FP_COL(B, j, a);
        len[j] = fp_norm3(a);
        longest = len[j] > longest ? len[j] : longest;
    }
    bool have[3];
    int n = 0;
    for (int j = 0; j < 3; ++j) {
        have[j] = len[j] > 1e-14 * longest;            // B was scaled to a largest entry of 1: no underflow above this
        n += have[j];
        for (int i = 0; i < 3; ++i) U[3 * i + j] = have[j] ? B[3 * i + j] / len[j] : 0.0;
    }
    if (n == 0) {
        for (int i = 0; i < 9; ++i) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else if (n < 3) {
        if (n == 1) {               // a second column: the axis least along the first, made orthogonal to it
            int j0 = have[0] ? 0 : have[1] ? 1 : 2, j1 = (j0 + 1) % 3;
            double u[3], e[3] = {0.0, 0.0, 0.0};
            FP_COL(U, j0, u);
            int ax = 0;
            for (int i = 1; i < 3; ++i) ax = fabs(u[i]) < fabs(u[ax]) ? i : ax;
            e[ax] = 1.0;
            const double along = u[ax];
            for (int i = 0; i < 3; ++i) e[i] -= along * u[i];
            const double l = fp_norm3(e);
            for (int i = 0; i < 3; ++i) U[3 * i + j1] = e[i] / l;
            have[j1] = true;
        }
        const int j2 = !have[0] ? 0 : !have[1] ? 1 : 2;         // the last column: the cross product of the other two, in cyclic order
        double a[3], b[3], r[3];
        FP_COL(U, (j2 + 1) % 3, a);
        FP_COL(U, (j2 + 2) % 3, b);
        fp_cross(a, b, r);
        for (int i = 0; i < 3; ++i) U[3 * i + j2] = r[i];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (U[3 * i] * W[3 * j] + U[3 * i + 1] * W[3 * j + 1]) + U[3 * i + 2] * W[3 * j + 2];
}

FA_HD double fp_det3(const double* m)
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// The ten corners of the pose box through P, moved so that the mean of the first four lies on the mean of landmarks 0..26
FA_HD void fp_box(const double P[12], const float* landmarks, int box[2 * FP_NBOX])
{
    const double rear = 90.0, front = 105.0, depth = 110.0;
    const double X[5] = {-1.0, -1.0, 1.0, 1.0, -1.0}, Y[5] = {-1.0, 1.0, 1.0, -1.0, -1.0};
    double pt[FP_NBOX][2], at[2], lm[2] = {0.0, 0.0};
    for (int i = 0; i < FP_NBOX; ++i) {
        const double size = i < 5 ? rear : front, z = i < 5 ? 0.0 : depth;
        for (int j = 0; j < 2; ++j)
            pt[i][j] = (((X[i % 5] * size) * P[4 * j] + (Y[i % 5] * size) * P[4 * j + 1]) + z * P[4 * j + 2]) + P[4 * j + 3];
    }
    for (int k = 0; k < 27; ++k) {
        lm[0] += (double)landmarks[3 * k];
        lm[1] += (double)landmarks[3 * k + 1];
    }
    for (int j = 0; j < 2; ++j) at[j] = (((pt[0][j] + pt[1][j]) + pt[2][j]) + pt[3][j]) / 4.0;
    for (int i = 0; i < FP_NBOX; ++i)
        for (int j = 0; j < 2; ++j) {
            const double v = (pt[i][j] - at[j]) + lm[j] / 27.0;
            box[2 * i + j] = !(v == v) ? 0 : (int)(v < -16384.0 ? -16384.0 : v > 16383.0 ? 16383.0 : v);
        }
}

// What an unused or invalid slot holds
FA_HD void fp_zero(FpPose* o)
{
    for (int i = 0; i < 12; ++i) o->P[i] = 0.0;
    o->angles[0] = o->angles[1] = o->angles[2] = o->scale = 0.0;
    for (int i = 0; i < 2 * FP_NBOX; ++i) o->box[i] = 0;
    o->valid = 0;
}

// A slot's results into the output arrays P [cap, 3, 4], angles [cap, 3], scale [cap], box [cap, 10, 2], valid [cap]
FA_HD void fp_store(const FpPose& o, int s, double* P, double* angles, double* scale, int* box, int* valid)
{
    for (int i = 0; i < 12; ++i) P[12 * (size_t)s + i] = o.P[i];
    for (int i = 0; i < 3; ++i) angles[3 * (size_t)s + i] = o.angles[i];
    scale[s] = o.scale;
    for (int i = 0; i < 2 * FP_NBOX; ++i) box[2 * FP_NBOX * (size_t)s + i] = o.box[i];
    valid[s] = o.valid;
}

// The moments of a slot (chunks already added up), its pivot, the canonical cloud's mean and rms_d1 (stats[0..2], stats[3]) and the
// slot's landmarks [68, 3] -> everything a FacePose holds for the slot
FA_HD void fp_solve(const double m[FP_NMOM], const double c[3], int V, const double stats[4], const float* landmarks, FpPose* o)
{
    fp_zero(o);
    bool finite = true;
    for (int k = 0; k < FP_NMOM; ++k) finite = finite && fp_finite(m[k]);
    if (!finite) return;
    const double n = (double)V, rms_d1 = stats[3];
    const double centred = (m[12] - ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) / n) / n;
    if (!(centred > 0.0) || !(rms_d1 > 0.0) || !fp_finite(rms_d1)) return;
    const double rms_d0 = sqrt(centred);
    if (!(rms_d0 > 0.0)) return;
    double R[9];
    fp_polar(m + 3, R);
    if (fp_det3(R) < 0.0)
        for (int i = 0; i < 3; ++i) R[3 * i + 2] = -R[3 * i + 2];
    const double s = rms_d0 / rms_d1;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o->P[4 * i + j] = s * R[3 * i + j];
        o->P[4 * i + 3] = (c[i] + m[i] / n) - stats[i];
    }
    o->scale = s;
    // P2sRt, matrix2angle
    double r1[3], r2[3], r3[3];
    const double n1 = fp_norm3(o->P), n2 = fp_norm3(o->P + 4);
    for (int j = 0; j < 3; ++j) {
        r1[j] = o->P[j] / n1;
        r2[j] = o->P[4 + j] / n2;
    }
    fp_cross(r1, r2, r3);
    const double sx = r3[0] < -1.0 ? -1.0 : r3[0] > 1.0 ? 1.0 : r3[0];
    const double x = asin(sx), cx = cos(x);
    o->angles[0] = x;
    o->angles[1] = atan2(r3[1] / cx, r3[2] / cx);
    o->angles[2] = atan2(r2[0] / cx, r1[0] / cx);
    fp_box(o->P, landmarks, o->box);
    o->valid = 1;
}
