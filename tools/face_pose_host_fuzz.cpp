// Host hygiene of the head-pose host twin: csrc/face_pose_host.h (the body of cp_face_pose_host) compiled with the host compiler under
// AddressSanitizer + UBSan and run over seeded fuzz cases -- vertex counts 3, 4, 255..257, 2047..2049, 5000; both sources (the plan's
// output restored on the fly, the restored map); capacities with unused slots; cells at the corners of the map, duplicates, and cells
// outside it (handed over directly: the slot must come out invalid, nothing outside the map is read); plan outputs that are NaN, +-inf,
// +-3e38; crop squares far away, hostile slots / xform; clouds that are one point, a line or a plane (rank 0, 1, 2 covariances); huge
// and tiny canonical clouds; landmarks that are NaN or +-3e38.  Every array lives in a heap block of exactly its size (anything past it
// is the sanitizer's redzone).  An unused or invalid slot must be all zeros with its scratch part untouched when unused; a valid slot
// must hold finite numbers, an orthogonal R of determinant +1 times a positive scale, angles within +-pi and a box inside -16384..16383.
// CPU only:   make -C centerpose_amd/csrc face_pose_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "face_pose_host.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static int g_failures = 0;
static long long g_valid = 0, g_invalid = 0, g_unused = 0;

#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            ++g_failures;                 \
        }                                 \
    } while (0)

static const float SPECIAL[] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e-30f, 0.f};
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))
static const double SENTINEL = -7.25;

static void run_case(int V, int from_pos, int shape)
{
    const int cap = 1 + rnd() % 4;
    const size_t map = (size_t)3 * FP_CELLS;
    std::unique_ptr<float[]> src(new float[cap * map]), xform(new float[3 * cap]), lm(new float[(size_t)cap * FA_NKPT * 3]);
    std::unique_ptr<int[]> slots(new int[cap]), ind(new int[V]), box(new int[(size_t)cap * 2 * FP_NBOX]), valid(new int[cap]);
    std::unique_ptr<double[]> canon(new double[3 * (size_t)V]), stats(new double[4]);
    const size_t nscratch = (size_t)cap * fp_slot_doubles(V);
    std::unique_ptr<double[]> scratch(new double[nscratch]), P(new double[12 * cap]), angles(new double[3 * cap]), scale(new double[cap]);
    for (size_t i = 0; i < nscratch; ++i) scratch[i] = SENTINEL;

    // shape 0: a volume, 1: every value the same (one point), 2: a line, 3: a plane, 4: hostile values sprinkled in
    for (int s = 0; s < cap; ++s)
        for (size_t i = 0; i < map; ++i) {
            const size_t cell = from_pos ? i / 3 : i % FP_CELLS, axis = from_pos ? i % 3 : i / FP_CELLS;
            float v = (float)uni(0, 1);
            if (shape == 1) v = 0.25f;
            if (shape == 2) v = (float)(cell % 977) / 977.f;
            if (shape == 3 && axis == 2) v = 0.5f;
            src[s * map + i] = v;
        }
    if (shape == 4)
        for (int k = 0; k < 3; ++k) src[rnd() % (cap * map)] = SPECIAL[rnd() % COUNT(SPECIAL)];
    for (int s = 0; s < cap; ++s) {
        slots[s] = (rnd() % 4 == 0) ? -1 : s;
        xform[3 * s] = (float)uni(-500, 8000); xform[3 * s + 1] = (float)uni(-500, 8000); xform[3 * s + 2] = (float)(1 + rnd() % 32768);
        if (rnd() % 8 == 0) {
            slots[s] = (rnd() % 2) ? FA_MAX_ROWS + (int)(rnd() % 3) : s;
            xform[3 * s + rnd() % 3] = SPECIAL[rnd() % COUNT(SPECIAL)];
        }
        for (int i = 0; i < FA_NKPT * 3; ++i) lm[(size_t)s * FA_NKPT * 3 + i] = (float)uni(-500, 9000);
        if (rnd() % 6 == 0) lm[(size_t)s * FA_NKPT * 3 + rnd() % 81] = SPECIAL[rnd() % COUNT(SPECIAL)];
    }
    bool outside = false;
    for (int v = 0; v < V; ++v) ind[v] = (int)(rnd() % FP_CELLS);
    ind[0] = FP_CELLS - 1; ind[V - 1] = 0; ind[1] = ind[2];
    if (rnd() % 6 == 0) {
        ind[rnd() % V] = (rnd() % 2) ? FP_CELLS + (int)(rnd() % 5) : -1 - (int)(rnd() % 5);
        outside = true;
    }
    const double spread = (rnd() % 5 == 0) ? 1e6 : (rnd() % 5 == 0) ? 1e-6 : 100.0;
    double mean[3] = {0, 0, 0}, ss = 0;
    for (int i = 0; i < 3 * V; ++i) canon[i] = uni(-spread, spread);
    if (shape == 3 && rnd() % 2)
        for (int v = 0; v < V; ++v) canon[3 * v + 1] = 0.0;
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < 3; ++k) mean[k] += canon[3 * v + k] / V;
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < 3; ++k) {
            canon[3 * v + k] -= mean[k];
            ss += canon[3 * v + k] * canon[3 * v + k];
        }
    stats[0] = mean[0]; stats[1] = mean[1]; stats[2] = mean[2]; stats[3] = sqrt(ss / V);

    char err[256];
    const int rc = fp_pose_host(src.get(), from_pos, slots.get(), xform.get(), cap, ind.get(), V, canon.get(), stats.get(), lm.get(),
                                scratch.get(), nscratch * sizeof(double), P.get(), angles.get(), scale.get(), box.get(), valid.get(), err,
                                sizeof(err));
    EXPECT(rc == 0, "refused: %s", err);
    if (rc) return;
    for (int s = 0; s < cap; ++s) {
        FaXform t;
        const bool used = fh_slot(slots.get(), xform.get(), s, 1, FA_MAX_ROWS, &t);
        const double* p = &P[12 * s];
        if (!used) {
            ++g_unused;
            for (size_t i = 0; i < fp_slot_doubles(V); ++i) EXPECT(scratch[s * fp_slot_doubles(V) + i] == SENTINEL, "unused slot %d: scratch written", s);
        }
        EXPECT(valid[s] == 0 || valid[s] == 1, "slot %d: valid = %d", s, valid[s]);
        EXPECT(used || !valid[s], "unused slot %d is valid", s);
        if (outside || shape == 1) EXPECT(!valid[s], "slot %d is valid (a cell outside the map: %d, one point: %d)", s, (int)outside, shape == 1);
        if (!valid[s]) {
            g_invalid += used;
            bool zero = scale[s] == 0.0;
            for (int i = 0; i < 12; ++i) zero = zero && p[i] == 0.0;
            for (int i = 0; i < 3; ++i) zero = zero && angles[3 * s + i] == 0.0;
            for (int i = 0; i < 2 * FP_NBOX; ++i) zero = zero && box[2 * FP_NBOX * s + i] == 0;
            EXPECT(zero, "slot %d is not valid and not all zeros", s);
            continue;
        }
        ++g_valid;
        bool finite = isfinite(scale[s]) && scale[s] > 0.0;
        for (int i = 0; i < 12; ++i) finite = finite && isfinite(p[i]);
        EXPECT(finite, "valid slot %d: P or scale not finite / positive", s);
        if (!finite) continue;
        double worst = 0.0;                                // (P[:, :3] / s) is orthogonal
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double dot = 0.0;
                for (int k = 0; k < 3; ++k) dot += p[4 * i + k] * p[4 * j + k];
                worst = fmax(worst, fabs(dot / (scale[s] * scale[s]) - (i == j ? 1.0 : 0.0)));
            }
        EXPECT(worst < 1e-12, "valid slot %d: R^T R is %.3e from the identity (shape %d, V %d)", s, worst, shape, V);
        const double R[9] = {p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]};
        EXPECT(fabs(fp_det3(R) / (scale[s] * scale[s] * scale[s]) - 1.0) < 1e-12, "valid slot %d: det R is not +1", s);
        for (int i = 0; i < 3; ++i) EXPECT(fabs(angles[3 * s + i]) <= 3.1415926535897936, "valid slot %d: angle %d = %g", s, i, angles[3 * s + i]);
        for (int i = 0; i < 2 * FP_NBOX; ++i)
            EXPECT(box[2 * FP_NBOX * s + i] >= -16384 && box[2 * FP_NBOX * s + i] <= 16383, "valid slot %d: box entry %d", s, box[2 * FP_NBOX * s + i]);
    }
}

int main()
{
    static const int VS[] = {3, 4, 255, 256, 257, 2047, 2048, 2049, 5000};
    int cases = 0;
    for (int rep = 0; rep < 4; ++rep)
        for (int V : VS)
            for (int from_pos = 0; from_pos < 2; ++from_pos)
                for (int shape = 0; shape < 5; ++shape, ++cases) run_case(V, from_pos, shape);
    // the polar factor of matrices of every rank, scaled up and down
    for (int k = 0; k < 4000; ++k) {
        double A[9], R[9];
        const int rank = k % 4;
        const double mag = (k % 3 == 0) ? 1e150 : (k % 3 == 1) ? 1e-150 : 1.0;
        double u[3][3], w[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { u[i][j] = uni(-1, 1); w[i][j] = uni(-1, 1); }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                A[3 * i + j] = 0.0;
                for (int r = 0; r < rank; ++r) A[3 * i + j] += mag * u[r][i] * w[r][j];
                if (rank == 3 && k % 8 == 3) A[3 * i + j] = (i == j) ? mag : 0.0;
            }
        fp_polar(A, R);
        double worst = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double dot = 0.0;
                for (int r = 0; r < 3; ++r) dot += R[3 * i + r] * R[3 * j + r];
                worst = fmax(worst, fabs(dot - (i == j ? 1.0 : 0.0)));
            }
        EXPECT(worst < 1e-12, "fp_polar: rank %d, magnitude %g: R^T R is %.3e from the identity", rank, mag, worst);
    }
    // refusals
    char err[256];
    double d[64];
    float f[4];
    int n[4];
    EXPECT(fp_pose_host(f, 1, n, f, 0, n, 3, d, d, f, d, sizeof(d), d, d, d, n, n, err, sizeof(err)) == 1, "capacity 0 accepted");
    EXPECT(fp_pose_host(f, 1, n, f, 1, n, 2, d, d, f, d, sizeof(d), d, d, d, n, n, err, sizeof(err)) == 1, "two vertices accepted");
    EXPECT(fp_pose_host(f, 1, n, f, 1, n, 65537, d, d, f, d, sizeof(d), d, d, d, n, n, err, sizeof(err)) == 1, "65537 vertices accepted");
    EXPECT(fp_pose_host(f, 1, n, f, 1, n, 3, d, d, f, d, 16 * 8 - 1, d, d, d, n, n, err, sizeof(err)) == 1, "short scratch accepted");
    EXPECT(fp_pose_host(f, 3, n, f, 1, n, 3, d, d, f, d, sizeof(d), d, d, d, n, n, err, sizeof(err)) == 1, "source kind 3 accepted");
    EXPECT(fp_pose_host(nullptr, 1, n, f, 1, n, 3, d, d, f, d, sizeof(d), d, d, d, n, n, err, sizeof(err)) == 1, "null source accepted");
    printf("face_pose_host_fuzz: %d cases, %lld valid slots, %lld invalid, %lld unused, %d failures\n", cases, g_valid, g_invalid, g_unused,
           g_failures);
    return g_failures ? 1 : 0;
}
