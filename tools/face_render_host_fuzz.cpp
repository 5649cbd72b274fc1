// Host hygiene of the mesh rasteriser's host twins: csrc/face_render_host.h (the bodies of cp_face_render_host and
// cp_face_vertex_colors[_yuv]_host) compiled with the host compiler under AddressSanitizer + UBSan and run over seeded fuzz cases --
// windows 1 x 1 .. 40 x 48 at origins up to +-2^20 (and one step beyond: the slot must come out unused); capacities with unused slots;
// vertices that are NaN, +-inf, +-3e38, +-1e30 and far outside the window; triangles larger than the window, degenerate ones,
// duplicates; C = 1..4 and the z attributes; frames in packed BGR with a padded pitch and in NV12 / P010 for the colours.  Every array
// lives in a heap block of exactly its size (anything past it is the sanitizer's redzone).  Checked: every key is 0 or names a
// triangle of the table that fr_setup accepts and fr_covers says covers the pixel, tri and image are what the key says, unused slots
// are all -1 / 0, and a second sweep with the triangles in reverse arrival order (the maximum of the same keys) gives the same keys.
// CPU only:   make -C centerpose_amd/csrc face_render_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "face_render_host.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static int g_failures = 0;
static long long g_covered = 0, g_empty = 0, g_unused = 0, g_colors = 0;

#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            ++g_failures;                 \
        }                                 \
    } while (0)

static const float SPECIAL[] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e30f, -1e30f, -999999.f, -0.f};
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

static void fill_maps(float* pos, int cap, const int* ind, int V, const int* origin, int h, int w)
{
    for (size_t i = 0; i < (size_t)cap * FR_CELLS * 3; ++i) pos[i] = (float)uni(-50, 50);
    for (int s = 0; s < cap; ++s)
        for (int k = 0; k < V; ++k) {
            float* p = pos + ((size_t)s * FR_CELLS + ind[k]) * 3;
            p[0] = (float)(origin[2 * s] + uni(-3, w + 3));
            p[1] = (float)(origin[2 * s + 1] + uni(-3, h + 3));
            if (rnd() % 4 == 0) { p[0] = rintf(p[0]); p[1] = rintf(p[1]); }
            p[2] = (float)(rnd() % 7) - 3.f;                                   // few depths: many ties
            if (rnd() % 40 == 0) p[rnd() % 3] = SPECIAL[rnd() % COUNT(SPECIAL)];
            if (rnd() % 50 == 0) { p[0] += (float)uni(-900, 900); p[1] += (float)uni(-900, 900); }
        }
}

static void run_render(int h, int w, int C, bool with_attrs)
{
    const int cap = 1 + rnd() % 3, V = 3 + rnd() % 200, T = 1 + rnd() % 400;
    const size_t window = (size_t)h * w;
    std::unique_ptr<float[]> pos(new float[(size_t)cap * FR_CELLS * 3]), attrs(new float[(size_t)cap * V * C]), image(new float[cap * window * C]);
    std::unique_ptr<int[]> slots(new int[cap]), ind(new int[V]), tri(new int[3 * (size_t)T]), origin(new int[2 * cap]), out_tri(new int[cap * window]);
    std::unique_ptr<uint64_t[]> keys(new uint64_t[cap * window]);
    for (int k = 0; k < V; ++k) ind[k] = (int)(rnd() % FR_CELLS);
    ind[0] = FR_CELLS - 1; ind[V - 1] = 0;
    for (int s = 0; s < cap; ++s) {
        slots[s] = (rnd() % 4 == 0) ? -1 - (int)(rnd() % 3) : (int)(rnd() % 1000);
        const int edge = rnd() % 6;
        origin[2 * s] = edge == 0 ? FR_MAX_ORIGIN : edge == 1 ? -FR_MAX_ORIGIN : (int)(rnd() % 4000) - 2000;
        origin[2 * s + 1] = edge == 2 ? FR_MAX_ORIGIN : edge == 3 ? -FR_MAX_ORIGIN : (int)(rnd() % 4000) - 2000;
        if (rnd() % 10 == 0) origin[2 * s + rnd() % 2] = (rnd() % 2) ? FR_MAX_ORIGIN + 1 : -FR_MAX_ORIGIN - 1;
    }
    fill_maps(pos.get(), cap, ind.get(), V, origin.get(), h, w);
    for (int i = 0; i < T; ++i) {
        const int a = rnd() % V, kind = rnd() % 8;
        tri[3 * i] = a;
        tri[3 * i + 1] = kind == 0 ? a : (int)(rnd() % V);
        tri[3 * i + 2] = kind == 1 ? tri[3 * i + 1] : (int)(rnd() % V);
        if (kind == 2 && i > 0) memcpy(&tri[3 * i], &tri[3 * (rnd() % i)], 3 * sizeof(int));
    }
    for (size_t i = 0; i < (size_t)cap * V * C; ++i) attrs[i] = (rnd() % 30 == 0) ? SPECIAL[rnd() % COUNT(SPECIAL)] : (float)uni(0, 255);

    char err[256];
    const int rc = fr_render_host(pos.get(), slots.get(), cap, ind.get(), V, tri.get(), T, origin.get(), h, w, with_attrs ? attrs.get() : nullptr,
                                  with_attrs ? C : 1, keys.get(), cap * window * 8, out_tri.get(), image.get(), err, sizeof(err));
    EXPECT(rc == 0, "refused: %s", err);
    if (rc) return;
    const int Cc = with_attrs ? C : 1;
    for (int s = 0; s < cap; ++s) {
        const bool used = fr_slot_used(slots.get(), origin.get(), s);
        g_unused += !used;
        const float* map = pos.get() + (size_t)s * FR_CELLS * 3;
        const int x0 = origin[2 * s], y0 = origin[2 * s + 1];
        // the same keys with the triangles arriving in reverse order
        std::vector<uint64_t> again(window, 0);
        if (used)
            for (int i = T - 1; i >= 0; --i) {
                const float* p[3];
                fr_gather(map, ind.get(), tri.get(), i, p);
                FrTri t;
                if (!fr_setup(p[0], p[1], p[2], x0, y0, h, w, &t)) continue;
                EXPECT(t.umin >= x0 && t.umax <= x0 + w - 1 && t.vmin >= y0 && t.vmax <= y0 + h - 1, "a box leaves the window");
                const uint64_t key = fr_key(t.d, i);
                EXPECT(key != 0 && fr_key_tri(key) == i, "key of triangle %d does not name it", i);
                for (int Y = t.vmin; Y <= t.vmax; ++Y)
                    for (int X = t.umin; X <= t.umax; ++X) {
                        uint64_t& k = again[(size_t)(Y - y0) * w + (X - x0)];
                        if (fr_covers(t, X, Y) && key > k) k = key;
                    }
            }
        for (size_t px = 0; px < window; ++px) {
            const size_t o = s * window + px;
            EXPECT(keys[o] == again[px], "slot %d pixel %zu: the key depends on the arrival order", s, px);
            EXPECT(out_tri[o] == fr_key_tri(keys[o]) && out_tri[o] >= -1 && out_tri[o] < T, "slot %d pixel %zu: tri %d", s, px, out_tri[o]);
            if (out_tri[o] < 0) {
                ++g_empty;
                for (int c = 0; c < Cc; ++c) EXPECT(image[o * Cc + c] == 0.f, "slot %d pixel %zu: an empty pixel is not 0", s, px);
            } else {
                ++g_covered;
                EXPECT(used, "unused slot %d holds a triangle", s);
            }
        }
    }
}

static void run_colors(int kind)
{
    const int cap = 1 + rnd() % 4, N = 1 + rnd() % cap, V = 3 + rnd() % 100, H = 2 * (1 + rnd() % 12), W = 2 * (1 + rnd() % 12);
    std::unique_ptr<float[]> pos(new float[(size_t)cap * FR_CELLS * 3]), colors(new float[(size_t)cap * V * 3]);
    std::unique_ptr<int[]> slots(new int[cap]), ind(new int[V]), origin(new int[2 * cap]);
    for (int k = 0; k < V; ++k) ind[k] = (int)(rnd() % FR_CELLS);
    for (int s = 0; s < cap; ++s) { slots[s] = (rnd() % 4 == 0) ? -1 : s; origin[2 * s] = origin[2 * s + 1] = 0; }
    fill_maps(pos.get(), cap, ind.get(), V, origin.get(), H, W);
    char err[256];
    int rc;
    std::vector<std::unique_ptr<unsigned char[]>> keep;
    if (kind == 0) {                                                   // packed BGR, 4 bytes per pixel, a padded pitch
        const long long pitch = 4 * W + 5;
        std::vector<RhFrameDesc> table(N);
        for (int n = 0; n < N; ++n) {
            const size_t bytes = (size_t)(H - 1) * pitch + (size_t)(W - 1) * 4 + 3;      // exactly the bytes the strides address
            keep.emplace_back(new unsigned char[bytes]);
            for (size_t i = 0; i < bytes; ++i) keep.back()[i] = (unsigned char)rnd();
            memset(&table[n], 0, sizeof(RhFrameDesc));
            table[n].base = keep.back().get();
            table[n].row_stride = pitch; table[n].pix_stride = 4;
            table[n].ch_off[0] = 0; table[n].ch_off[1] = 1; table[n].ch_off[2] = 2;
            table[n].H = H; table[n].W = W;
        }
        rc = fr_colors_host(table.data(), N, pos.get(), slots.get(), cap, ind.get(), V, colors.get(), err, sizeof(err));
    } else {                                                           // NV12 (8-bit) or P010 (16-bit containers): two planes
        const int b = kind == 1 ? 1 : 2;
        const int coef[6] = {1220542, 1673527, -852492, -409993, 2116026, 16};
        std::vector<RhYuvFrameDesc> table(N);
        for (int n = 0; n < N; ++n) {
            const size_t ybytes = (size_t)H * W * b, cbytes = (size_t)(H / 2) * W * b;
            keep.emplace_back(new unsigned char[ybytes]);
            unsigned char* y = keep.back().get();
            keep.emplace_back(new unsigned char[cbytes]);
            unsigned char* c = keep.back().get();
            for (size_t i = 0; i < ybytes; ++i) y[i] = (unsigned char)rnd();
            for (size_t i = 0; i < cbytes; ++i) c[i] = (unsigned char)rnd();
            memset(&table[n], 0, sizeof(RhYuvFrameDesc));
            table[n].y_base = y; table[n].y_row = (long long)W * b; table[n].y_pix = b;
            table[n].u_base = c; table[n].v_base = c + b; table[n].c_row = (long long)W * b; table[n].c_pix = 2 * b;
            table[n].H = H; table[n].W = W;
            table[n].pad = kind == 1 ? 0 : YS_16BIT;
        }
        rc = fr_colors_yuv_host(table.data(), N, coef, pos.get(), slots.get(), cap, ind.get(), V, colors.get(), err, sizeof(err));
    }
    EXPECT(rc == 0, "colours refused: %s", err);
    if (rc) return;
    const int q = cap / N;
    for (int s = 0; s < cap; ++s)
        for (int k = 0; k < 3 * V; ++k) {
            const float c = colors[(size_t)s * V * 3 + k];
            ++g_colors;
            EXPECT(c >= 0.f && c <= 255.f && c == rintf(c), "slot %d: colour %g", s, (double)c);
            if (slots[s] < 0 || s / q >= N) EXPECT(c == 0.f, "unused slot %d has a colour", s);
        }
}

int main()
{
    static const int SIZES[][2] = {{1, 1}, {1, 7}, {5, 1}, {21, 27}, {33, 65}, {40, 48}};
    int cases = 0;
    for (int rep = 0; rep < 6; ++rep)
        for (const auto& hw : SIZES)
            for (int C = 1; C <= FR_MAX_C; ++C, ++cases) run_render(hw[0], hw[1], C, (C + rep) % 5 != 0);
    for (int rep = 0; rep < 60; ++rep, ++cases) run_colors(rep % 3);
    // refusals
    char err[256];
    float f[16];
    int n[16] = {0};
    uint64_t k[16];
    EXPECT(fr_render_host(f, n, 0, n, 3, n, 1, n, 1, 1, f, 1, k, sizeof(k), n, f, err, sizeof(err)) == 1, "capacity 0 accepted");
    EXPECT(fr_render_host(f, n, 1, n, 2, n, 1, n, 1, 1, f, 1, k, sizeof(k), n, f, err, sizeof(err)) == 1, "two vertices accepted");
    EXPECT(fr_render_host(f, n, 1, n, 3, n, 0, n, 1, 1, f, 1, k, sizeof(k), n, f, err, sizeof(err)) == 1, "no triangle accepted");
    EXPECT(fr_render_host(f, n, 1, n, 3, n, 1, n, 0, 1, f, 1, k, sizeof(k), n, f, err, sizeof(err)) == 1, "empty window accepted");
    EXPECT(fr_render_host(f, n, 1, n, 3, n, 1, n, 1, 4097, f, 1, k, 1 << 20, n, f, err, sizeof(err)) == 1, "window of 4097 accepted");
    EXPECT(fr_render_host(f, n, 16, n, 3, n, 1, n, 4096, 4096, f, 1, k, (size_t)1 << 40, n, f, err, sizeof(err)) == 1, "2^31 bytes of keys accepted");
    EXPECT(fr_render_host(f, n, 1, n, 3, n, 1, n, 1, 1, f, 5, k, sizeof(k), n, f, err, sizeof(err)) == 1, "five channels accepted");
    EXPECT(fr_render_host(f, n, 1, n, 3, n, 1, n, 1, 1, nullptr, 2, k, sizeof(k), n, f, err, sizeof(err)) == 1, "z with two channels accepted");
    EXPECT(fr_render_host(f, n, 1, n, 3, n, 1, n, 2, 2, f, 1, k, 31, n, f, err, sizeof(err)) == 1, "short scratch accepted");
    EXPECT(fr_render_host(nullptr, n, 1, n, 3, n, 1, n, 1, 1, f, 1, k, sizeof(k), n, f, err, sizeof(err)) == 1, "null maps accepted");
    n[1] = 3;
    EXPECT(fr_render_host(f, n + 4, 1, n + 4, 3, n, 1, n + 4, 1, 1, f, 1, k, sizeof(k), n + 8, f, err, sizeof(err)) == 1, "vertex 3 of 3 accepted");
    n[1] = FR_CELLS;
    EXPECT(fr_render_host(f, n + 4, 1, n, 3, n + 4, 1, n + 4, 1, 1, f, 1, k, sizeof(k), n + 8, f, err, sizeof(err)) == 1, "cell 65536 accepted");
    printf("face_render_host_fuzz: %d cases, %lld covered pixels, %lld empty, %lld unused slots, %lld colours, %d failures\n", cases, g_covered,
           g_empty, g_unused, g_colors, g_failures);
    return g_failures ? 1 : 0;
}
