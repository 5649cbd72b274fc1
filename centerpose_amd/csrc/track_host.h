// Sequential HOST twins of the track-association stage (track_assoc.hip) and the rectangular assignment, plain C++: compiled into the
// library (cp_track_*_host, cp_linear_assignment_host) and into the host-only fuzz program (tools/track_host_fuzz.cpp).
//
// The inverse-norm rule is shared with the append kernel through th_tree_sumsq / th_inv_norm below: the squares of 512 floats are
// summed in double in ONE fixed order (lane i of 128 takes elements 4i..4i+3 left to right, then a halving tree over the 128
// partials), rounded to float, and the result is 1.0f / sqrtf(that) -- so the device and the host write the same bits.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#define TH_DIM 512            // feature length (Net(reid=True): model.py:49-93)
#define TH_MAX_BUDGET 128     // ring rows per track slot: four 32-row MFMA slices
#define TH_MAX_TCAP 1024
#define TH_LANES 128          // TH_DIM / 4: one float4 per lane of the append block

#ifdef __HIPCC__
#define TH_HD __host__ __device__
#else
#define TH_HD
#endif

TH_HD static inline float th_inv_norm(double sumsq) { return 1.0f / sqrtf((float)sumsq); }

// the four squares of one lane, left to right, in double (every product is exact: 24 x 24 bits)
TH_HD static inline double th_lane_sumsq(float a, float b, float c, float d)
{
    return (((double)a * (double)a + (double)b * (double)b) + (double)c * (double)c) + (double)d * (double)d;
}

static inline double th_tree_sumsq(const float* x)
{
    double p[TH_LANES];
    for (int i = 0; i < TH_LANES; ++i) p[i] = th_lane_sumsq(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
    for (int s = TH_LANES / 2; s >= 1; s >>= 1)
        for (int i = 0; i < s; ++i) p[i] += p[i + s];
    return p[0];
}

#define TH_FAIL(...)                         \
    do {                                     \
        snprintf(err, errn, __VA_ARGS__);    \
        return 1;                            \
    } while (0)

// what both cost entry points refuse (pointers apart)
static inline int th_check_cost(const char* who, int M, int S, int Tcap, int budget, int q, char* err, size_t errn)
{
    if (budget < 1 || budget > TH_MAX_BUDGET) TH_FAIL("%s: budget %d outside 1..%d", who, budget, TH_MAX_BUDGET);
    if (Tcap < 1 || Tcap > TH_MAX_TCAP) TH_FAIL("%s: Tcap %d outside 1..%d", who, Tcap, TH_MAX_TCAP);
    if (q < 1) TH_FAIL("%s: q = %d: every stream needs at least one detection slot", who, q);
    if (S < 1 || S > 65535) TH_FAIL("%s: S = %d outside 1..65535", who, S);
    if (M < 0) TH_FAIL("%s: M = %d is negative", who, M);
    // ring rows, detection slots and detection rows are indexed in int; the float offsets built from them are size_t
    if ((long long)S * Tcap * budget > 0x7fffffffll)
        TH_FAIL("%s: S * Tcap * budget = %lld ring rows (x %d floats) exceed the 2^31 - 1 rows the index arithmetic holds", who,
                (long long)S * Tcap * budget, TH_DIM);
    if ((long long)S * q > (1ll << 24)) TH_FAIL("%s: S * q = %lld detection slots exceed 2^24", who, (long long)S * q);
    if ((long long)S * M > (1ll << 24)) TH_FAIL("%s: S * M = %lld rows exceed 2^24", who, (long long)S * M);
    return 0;
}

static inline int th_cost_host(const float* gallery, const float* ginv, const int* glen, const float* features, const int* slots,
                               const float* rows, int M, int S, int Tcap, int budget, int q, float* out, char* err, size_t errn)
{
    const char* who = "track_cost_host";
    if (int rc = th_check_cost(who, M, S, Tcap, budget, q, err, errn)) return rc;
    if (!gallery || !ginv || !glen || !features || !slots || !out || (!rows && M > 0)) TH_FAIL("%s: null pointer", who);
    const float inf = std::numeric_limits<float>::infinity();
    float* cost = out;
    float* det = out + (size_t)S * Tcap * q;
    std::vector<float> finv((size_t)q);
    for (int s = 0; s < S; ++s) {
        for (int d = 0; d < q; ++d) {
            const int v = slots[(size_t)s * q + d];
            const bool used = v >= 0 && (long long)v < (long long)S * M;
            float* o = det + ((size_t)s * q + d) * 5;
            for (int k = 0; k < 5; ++k) o[k] = used ? rows[(size_t)v * 56 + k] : 0.f;
            finv[d] = used ? th_inv_norm(th_tree_sumsq(features + ((size_t)s * q + d) * TH_DIM)) : 0.f;
        }
        for (int t = 0; t < Tcap; ++t) {
            const size_t slot = (size_t)s * Tcap + t;
            int n = glen[slot];
            if (n > budget) n = budget;
            for (int d = 0; d < q; ++d) {
                float best = inf;
                const bool used = slots[(size_t)s * q + d] >= 0 && (long long)slots[(size_t)s * q + d] < (long long)S * M;
                if (used) {
                    const float* f = features + ((size_t)s * q + d) * TH_DIM;
                    for (int g = 0; g < n; ++g) {
                        const float* a = gallery + (slot * budget + g) * TH_DIM;
                        float acc = 0.f;
                        for (int k = 0; k < TH_DIM; ++k) acc += a[k] * f[k];
                        const float c = 1.f - acc * ginv[slot * budget + g] * finv[d];
                        if (c < best) best = c;
                    }
                }
                cost[slot * q + d] = best;
            }
        }
    }
    return 0;
}

static inline int th_append_host(float* gallery, float* ginv, const float* features, const int* table, int n, int budget, char* err,
                                 size_t errn)
{
    const char* who = "track_append_host";
    if (budget < 1 || budget > TH_MAX_BUDGET) TH_FAIL("%s: budget %d outside 1..%d", who, budget, TH_MAX_BUDGET);
    if (n < 0 || n > (1 << 24)) TH_FAIL("%s: n = %d outside 0..2^24", who, n);
    if (!gallery || !ginv || !features || (!table && n > 0)) TH_FAIL("%s: null pointer", who);
    for (int i = 0; i < n; ++i) {
        const int fs = table[3 * i], ts = table[3 * i + 1], pos = table[3 * i + 2];
        if (fs < 0 || ts < 0 || pos < 0 || pos >= budget) continue;          // as the kernel: such an entry writes nothing
        const float* f = features + (size_t)fs * TH_DIM;
        const size_t row = (size_t)ts * budget + pos;
        memcpy(gallery + row * TH_DIM, f, TH_DIM * sizeof(float));
        ginv[row] = th_inv_norm(th_tree_sumsq(f));
    }
    return 0;
}

// Per-row track ids: row_ids[S, M] = -1 everywhere, then row_ids[slots[i]] = slot_ids[i] for every detection slot i < S * q that is used
// (slots[i] >= 0) and matched (slot_ids[i] >= 0).  What both entry points refuse (pointers and slot values apart):
static inline int th_check_row_ids(const char* who, int capacity, int S, int q, int M, char* err, size_t errn)
{
    if (S < 1 || S > 65535) TH_FAIL("%s: S = %d outside 1..65535", who, S);
    if (q < 1) TH_FAIL("%s: q = %d: every stream needs at least one detection slot", who, q);
    if (M < 0) TH_FAIL("%s: M = %d is negative", who, M);
    if ((long long)S * q > (1ll << 24)) TH_FAIL("%s: S * q = %lld detection slots exceed 2^24", who, (long long)S * q);
    if ((long long)capacity < (long long)S * q) TH_FAIL("%s: capacity %d holds fewer than S * q = %lld slots", who, capacity, (long long)S * q);
    if ((long long)S * M > (1ll << 24)) TH_FAIL("%s: S * M = %lld rows exceed 2^24", who, (long long)S * M);
    return 0;
}

static inline int th_row_ids_host(const int* slots, const int* slot_ids, int capacity, int S, int q, int M, int* row_ids, char* err,
                                  size_t errn)
{
    const char* who = "track_row_ids_host";
    if (int rc = th_check_row_ids(who, capacity, S, q, M, err, errn)) return rc;
    if (!slots || !slot_ids || (!row_ids && M > 0)) TH_FAIL("%s: null pointer", who);
    const int total = S * M;
    for (int i = 0; i < S * q; ++i)
        if (slots[i] < -1 || slots[i] >= total) TH_FAIL("%s: slot %d holds row %d outside -1..%d", who, i, slots[i], total - 1);
    for (int r = 0; r < total; ++r) row_ids[r] = -1;
    for (int i = 0; i < S * q; ++i)
        if (slots[i] >= 0 && slot_ids[i] >= 0) row_ids[slots[i]] = slot_ids[i];
    return 0;
}

// Rectangular minimum-cost assignment on float64: shortest augmenting paths with row / column potentials (the Hungarian method in
// its O(n^2 m) form; Kuhn 1955, Munkres 1957, Jonker & Volgenant 1987 for the potentials).  min(rows, cols) pairs are made;
// row_to_col[r] is the column of row r or -1.  Entries must be finite.
static inline int th_linear_assignment(const double* cost, int rows, int cols, int ld, int* row_to_col, char* err, size_t errn)
{
    const char* who = "linear_assignment_host";
    if (rows < 0 || cols < 0 || rows > 4096 || cols > 4096) TH_FAIL("%s: %d x %d outside 0..4096", who, rows, cols);
    if (rows > 0 && (!cost || !row_to_col)) TH_FAIL("%s: null pointer", who);
    if (ld < cols) TH_FAIL("%s: ld %d < cols %d", who, ld, cols);
    for (int r = 0; r < rows; ++r) {
        row_to_col[r] = -1;
        for (int c = 0; c < cols; ++c)
            if (!isfinite(cost[(size_t)r * ld + c])) TH_FAIL("%s: entry (%d, %d) is not finite", who, r, c);
    }
    if (rows == 0 || cols == 0) return 0;
    // the path search runs over the SHORTER side as "workers" (n) and the longer one as "jobs" (m)
    const bool flip = rows > cols;
    const int n = flip ? cols : rows, m = flip ? rows : cols;
    auto at = [&](int i, int j) { return flip ? cost[(size_t)j * ld + i] : cost[(size_t)i * ld + j]; };
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u((size_t)n + 1, 0.0), v((size_t)m + 1, 0.0), minv((size_t)m + 1);
    std::vector<int> p((size_t)m + 1, 0), way((size_t)m + 1, 0);      // p[j]: worker (1-based) holding job j, 0 = free
    std::vector<char> used((size_t)m + 1);
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        for (int j = 0; j <= m; ++j) minv[j] = inf, used[j] = 0;
        do {
            used[j0] = 1;
            const int i0 = p[j0];
            double delta = inf;
            int j1 = 0;
            for (int j = 1; j <= m; ++j) {
                if (used[j]) continue;
                const double cur = at(i0 - 1, j - 1) - u[i0] - v[j];
                if (cur < minv[j]) minv[j] = cur, way[j] = j0;
                if (minv[j] < delta) delta = minv[j], j1 = j;
            }
            for (int j = 0; j <= m; ++j) {
                if (used[j]) u[p[j]] += delta, v[j] -= delta;
                else minv[j] -= delta;
            }
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    for (int j = 1; j <= m; ++j) {
        if (!p[j]) continue;
        if (flip) row_to_col[j - 1] = p[j] - 1;
        else row_to_col[p[j] - 1] = j - 1;
    }
    return 0;
}
