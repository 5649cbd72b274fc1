// Host hygiene of the track-association host twins and the assignment: csrc/track_host.h (the bodies of cp_track_cost_host,
// cp_track_append_host and cp_linear_assignment_host) compiled with the host compiler under AddressSanitizer + UBSan and run over seeded
// fuzz cases -- S 1..3, Tcap 1..5, budget 1..9, q 1..7, glen from negative to beyond the budget, slots that are -1, out of range or
// valid, append tables with negative indices and positions at and beyond the budget; assignment matrices 0x0 .. 9x9 with a row stride
// beyond the columns, thresholded ties, and every refusal.  Every array lives in a heap block of exactly its size (anything past it is
// the sanitizer's redzone).  The assignment is checked against a brute-force search over all injections.
// CPU only:   make -C centerpose_amd/csrc track_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <vector>
#include "track_host.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static int g_failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            ++g_failures;                 \
        }                                 \
    } while (0)

template <class T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

static void fuzz_cost_append(int iter)
{
    char err[256];
    const int S = 1 + rnd() % 3, Tcap = 1 + rnd() % 5, budget = 1 + rnd() % 9, q = 1 + rnd() % 7, M = rnd() % 6;
    const size_t nslot = (size_t)S * Tcap, nrow = nslot * budget, ndet = (size_t)S * q;
    auto gallery = block<float>(nrow * TH_DIM);
    auto ginv = block<float>(nrow);
    auto glen = block<int>(nslot);
    auto features = block<float>(ndet * TH_DIM);
    auto slots = block<int>(ndet);
    auto rows = block<float>((size_t)S * M * 56);
    auto out = block<float>(nslot * q + ndet * 5);
    for (size_t i = 0; i < nrow * TH_DIM; ++i) gallery[i] = (float)uni(-2, 2);
    for (size_t i = 0; i < nrow; ++i) ginv[i] = (float)uni(0.01, 1);
    for (size_t i = 0; i < nslot; ++i) glen[i] = (int)(rnd() % (budget + 4)) - 1;
    for (size_t i = 0; i < ndet * TH_DIM; ++i) features[i] = (float)uni(-2, 2);
    for (size_t i = 0; i < ndet; ++i) slots[i] = (int)(rnd() % (S * M + 3)) - 1;
    for (size_t i = 0; i < (size_t)S * M * 56; ++i) rows[i] = (float)uni(-50, 700);
    int rc = th_cost_host(gallery.get(), ginv.get(), glen.get(), features.get(), slots.get(), M ? rows.get() : nullptr, M, S, Tcap, budget, q,
                          out.get(), err, sizeof(err));
    EXPECT(rc == 0, "iter %d: cost rc %d (%s)", iter, rc, err);
    for (int s = 0; s < S; ++s)
        for (int t = 0; t < Tcap; ++t)
            for (int d = 0; d < q; ++d) {
                const int v = slots[(size_t)s * q + d];
                const bool live = v >= 0 && v < S * M && glen[(size_t)s * Tcap + t] > 0;
                const float c = out[((size_t)s * Tcap + t) * q + d];
                EXPECT(live ? isfinite(c) : (isinf(c) && c > 0), "iter %d: cost[%d,%d,%d] = %g, live %d", iter, s, t, d, c, (int)live);
            }
    // append: a table with good and bad entries
    const int n = rnd() % 6;
    auto table = block<int>((size_t)n * 3);
    for (int i = 0; i < n; ++i) {
        table[3 * i] = (int)(rnd() % (ndet + 1)) - 1;
        table[3 * i + 1] = (int)(rnd() % (nslot + 1)) - 1;
        table[3 * i + 2] = (int)(rnd() % (budget + 2)) - 1;
    }
    rc = th_append_host(gallery.get(), ginv.get(), features.get(), n ? table.get() : nullptr, n, budget, err, sizeof(err));
    EXPECT(rc == 0, "iter %d: append rc %d (%s)", iter, rc, err);
    for (int i = n - 1; i >= 0; --i) {
        const int fs = table[3 * i], ts = table[3 * i + 1], pos = table[3 * i + 2];
        if (fs < 0 || ts < 0 || pos < 0 || pos >= budget) continue;
        bool later = false;                 // a later entry may have overwritten the same ring row
        for (int j = i + 1; j < n; ++j) later |= table[3 * j] >= 0 && table[3 * j + 1] == ts && table[3 * j + 2] == pos;
        if (later) continue;
        const size_t row = (size_t)ts * budget + pos;
        EXPECT(memcmp(&gallery[row * TH_DIM], &features[(size_t)fs * TH_DIM], TH_DIM * sizeof(float)) == 0, "iter %d: ring row differs", iter);
        double ss = 0;
        for (int k = 0; k < TH_DIM; ++k) ss += (double)features[(size_t)fs * TH_DIM + k] * features[(size_t)fs * TH_DIM + k];
        EXPECT(fabs(ginv[row] * sqrt(ss) - 1.0) < 1e-6, "iter %d: ginv %g for |f| %g", iter, ginv[row], sqrt(ss));
    }
}

static double brute(const double* c, int rows, int cols, int ld)
{
    // the cheapest injection of the shorter side into the longer one
    const bool flip = rows > cols;
    const int n = flip ? cols : rows, m = flip ? rows : cols;
    std::vector<int> pick(m);
    for (int j = 0; j < m; ++j) pick[j] = j;
    double best = INFINITY;
    std::vector<int> sel(n);
    // all ordered n-subsets of m through permutations of a 0/1 mask and of the selection
    std::vector<int> mask(m, 0);
    std::fill(mask.end() - n, mask.end(), 1);
    do {
        int k = 0;
        for (int j = 0; j < m; ++j)
            if (mask[j]) sel[k++] = j;
        do {
            double tot = 0;
            for (int i = 0; i < n; ++i) tot += flip ? c[(size_t)sel[i] * ld + i] : c[(size_t)i * ld + sel[i]];
            best = std::min(best, tot);
        } while (std::next_permutation(sel.begin(), sel.end()));
    } while (std::next_permutation(mask.begin(), mask.end()));
    return best;
}

static void fuzz_assignment(int iter)
{
    char err[256];
    const int rows = rnd() % 7, cols = rnd() % 7, ld = cols + rnd() % 3;
    auto cost = block<double>((size_t)rows * ld);
    auto r2c = block<int>(rows);
    const bool capped = rnd() % 2;
    for (size_t i = 0; i < (size_t)rows * ld; ++i) {
        cost[i] = uni(0, 1);
        if (capped && cost[i] > 0.3) cost[i] = 0.3 + 1e-5;
    }
    int rc = th_linear_assignment(cost.get(), rows, cols, ld, r2c.get(), err, sizeof(err));
    EXPECT(rc == 0, "iter %d: assignment rc %d (%s)", iter, rc, err);
    std::vector<int> seen(cols, 0);
    int pairs = 0;
    double tot = 0;
    for (int r = 0; r < rows; ++r) {
        if (r2c[r] < 0) continue;
        EXPECT(r2c[r] < cols && !seen[r2c[r]], "iter %d: column %d taken twice or out of range", iter, r2c[r]);
        if (r2c[r] < cols) seen[r2c[r]] = 1, tot += cost[(size_t)r * ld + r2c[r]];
        ++pairs;
    }
    EXPECT(pairs == std::min(rows, cols), "iter %d: %d pairs for %d x %d", iter, pairs, rows, cols);
    if (rows && cols) {
        const double want = brute(cost.get(), rows, cols, ld);
        EXPECT(fabs(tot - want) <= 1e-12, "iter %d: total %.17g, brute force %.17g (%d x %d)", iter, tot, want, rows, cols);
    }
}

static void refusals()
{
    char err[256];
    float f[4] = {0};
    int i[4] = {0};
    double c[4] = {0, 1, NAN, 3};
    EXPECT(th_check_cost("t", 1, 1, 1, 0, 1, err, sizeof(err)) == 1, "budget 0");
    EXPECT(th_check_cost("t", 1, 1, 1, 129, 1, err, sizeof(err)) == 1, "budget 129");
    EXPECT(th_check_cost("t", 1, 1, 0, 1, 1, err, sizeof(err)) == 1, "Tcap 0");
    EXPECT(th_check_cost("t", 1, 1, 1025, 1, 1, err, sizeof(err)) == 1, "Tcap 1025");
    EXPECT(th_check_cost("t", 1, 1, 1, 1, 0, err, sizeof(err)) == 1, "q 0");
    EXPECT(th_check_cost("t", 1, 20000, 1024, 128, 1, err, sizeof(err)) == 1, "too many ring rows");
    EXPECT(th_check_cost("t", 1, 16383, 1024, 128, 1, err, sizeof(err)) == 0, "the largest gallery");
    EXPECT(th_cost_host(nullptr, f, i, f, i, f, 1, 1, 1, 1, 1, f, err, sizeof(err)) == 1, "null gallery");
    EXPECT(th_append_host(f, f, f, nullptr, 1, 1, err, sizeof(err)) == 1, "null table");
    EXPECT(th_append_host(f, f, f, i, -1, 1, err, sizeof(err)) == 1, "negative n");
    EXPECT(th_linear_assignment(c, 2, 2, 2, i, err, sizeof(err)) == 1, "NaN entry");
    EXPECT(th_linear_assignment(c, 1, 2, 1, i, err, sizeof(err)) == 1, "ld < cols");
    EXPECT(th_linear_assignment(nullptr, 0, 0, 0, nullptr, err, sizeof(err)) == 0, "0 x 0");
}

int main()
{
    for (int it = 0; it < 300; ++it) fuzz_cost_append(it);
    for (int it = 0; it < 3000; ++it) fuzz_assignment(it);
    refusals();
    printf("track_host_fuzz: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
