// Host hygiene of the re-id crop host twins: csrc/reid_host.h (the bodies of cp_reid_select_rows_host, cp_reid_crop_frames_host and
// cp_reid_crop_yuv_frames_host) compiled with the host compiler under AddressSanitizer + UBSan and run over seeded fuzz cases --
// frame sizes 1x1, 2x2, 7x5, 37x53, 64x64; packed / 4-channel / padded / planar BGR and RGB views; NV12 / NV21 / I420 planes, pitched,
// odd sizes; rows with boxes far outside, reversed, empty, +-1e9, +-3e9, NaN, +-inf, scores at the threshold and NaN; capacities
// with and without spare slots.  Every frame lives in a heap block of exactly its span (anything past it is the sanitizer's redzone:
// a tap outside the crop's frame is caught), slots / counts / out in blocks of exactly their size; frames must come back unchanged,
// every slot must name a selected row of its own frame or be -1 with an all-zero crop, and no output may be NaN or infinite.
// CPU only:   make -C centerpose_amd/csrc reid_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "reid_host.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static int g_failures = 0;
static long long g_crops = 0, g_empty = 0;

#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            ++g_failures;                 \
        }                                 \
    } while (0)

struct Block {
    std::unique_ptr<unsigned char[]> buf, orig;
    size_t size = 0;
    void alloc(size_t n)
    {
        size = n;
        buf.reset(new unsigned char[n]);
        orig.reset(new unsigned char[n]);
        for (size_t i = 0; i < n; ++i) buf[i] = orig[i] = (unsigned char)rnd();
    }
    bool same() const { return memcmp(buf.get(), orig.get(), size) == 0; }
};

static const float SPECIAL[] = {1e9f, -1e9f, 3e9f, -3e9f, NAN, INFINITY, -INFINITY, 1073741824.f, -1073741824.f};
static const float SCORES[] = {1.f, 0.5f, 0.3f, 0.30000004f, 1e-30f, 0.f, -1.f, NAN, INFINITY};

static std::vector<float> fuzz_rows(int N, int M, int H, int W)
{
    std::vector<float> rows((size_t)N * M * RA_ROW, 0.f);
    for (int r = 0; r < N * M; ++r) {
        float* row = &rows[(size_t)r * RA_ROW];
        const double cx = uni(-W, 2 * W), cy = uni(-H, 2 * H), w = uni(-2, W + 6), h = uni(-2, H + 6);
        row[0] = (float)(cx - w / 2); row[1] = (float)(cy - h / 2); row[2] = (float)(cx + w / 2); row[3] = (float)(cy + h / 2);
        if (rnd() % 5 == 0) row[rnd() % 4] = SPECIAL[rnd() % (sizeof(SPECIAL) / sizeof(SPECIAL[0]))];
        row[4] = SCORES[rnd() % (sizeof(SCORES) / sizeof(SCORES[0]))];
    }
    return rows;
}

template <class Desc>
static void check_result(const char* what, const Desc* table, int N, const std::vector<float>& rows, int M, float vis, int cap, const int* slots,
                         const int* counts, const float* out)
{
    const int q = cap / N;
    const size_t crop = (size_t)3 * RA_OUT_H * RA_OUT_W;
    for (int n = 0; n < N; ++n) {
        int c = 0;
        for (int m = 0; m < M; ++m) {
            RaBox b;
            if (ra_select(&rows[((size_t)n * M + m) * RA_ROW], vis, table[n].H, table[n].W, &b)) {
                EXPECT(b.x1 >= 0 && b.y1 >= 0 && b.x2 <= table[n].W - 1 && b.y2 <= table[n].H - 1 && b.x2 > b.x1 && b.y2 > b.y1,
                       "%s: crop (%d, %d, %d, %d) leaves the %d x %d frame", what, b.x1, b.y1, b.x2, b.y2, table[n].H, table[n].W);
                ++c;
            }
        }
        EXPECT(counts[n] == c, "%s: frame %d counts %d, %d rows are selected", what, n, counts[n], c);
    }
    for (int s = 0; s < cap; ++s) {
        const float* o = out + (size_t)s * crop;
        bool any = false, finite = true;
        for (size_t i = 0; i < crop; ++i) {
            any = any || o[i] != 0.f;
            finite = finite && isfinite(o[i]);
        }
        EXPECT(finite, "%s: slot %d holds a value that is not finite", what, s);
        if (slots[s] < 0) {
            EXPECT(!any, "%s: unused slot %d is not all zeros", what, s);
            ++g_empty;
        } else {
            EXPECT(s < N * q && slots[s] / M == s / q, "%s: slot %d names row %d of another frame", what, s, slots[s]);
            ++g_crops;
        }
    }
}

static RaNorm fuzz_norm()
{
    RaNorm nm = {rnd() & 1 ? 1.f : 1.f / 255.f, {0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, (int)(rnd() & 1)};
    return nm;
}

static void run_bgr(int H, int W, int N, int M, int cap)
{
    std::vector<Block> blocks(N);
    std::vector<RhFrameDesc> table(N);
    for (int n = 0; n < N; ++n) {
        const int form = rnd() % 4;
        RhFrameDesc d;
        memset(&d, 0, sizeof(d));
        d.H = H; d.W = W; d.NH = H; d.NW = W; d.mid_off = -1;
        const bool rgb = rnd() & 1;
        long long chs;
        if (form == 0) { d.pix_stride = 3; d.row_stride = 3ll * W; chs = 1; }                      // packed
        else if (form == 1) { d.pix_stride = 4; d.row_stride = 4ll * W + 13; chs = 1; }            // 4 channels, padded rows
        else if (form == 2) { d.pix_stride = 1; d.row_stride = W; chs = (long long)H * W; }        // planar
        else { d.pix_stride = 1; d.row_stride = W + 5; chs = (long long)H * (W + 5) + 9; }         // planar, padded rows and planes
        for (int k = 0; k < 3; ++k) d.ch_off[k] = (rgb ? 2 - k : k) * chs;
        const size_t span = (size_t)((H - 1) * d.row_stride + (W - 1) * d.pix_stride + 2 * chs + 1);
        blocks[n].alloc(span);
        d.base = blocks[n].buf.get();
        table[n] = d;
    }
    const std::vector<float> rows = fuzz_rows(N, M, H, W);
    std::unique_ptr<int[]> slots(new int[cap]), counts(new int[N]);
    std::unique_ptr<float[]> out(new float[(size_t)cap * 3 * RA_OUT_H * RA_OUT_W]);
    char err[256];
    const RaNorm nm = fuzz_norm();
    int rc = rh_select_host(table.data(), 0, N, rows.data(), M, 0.3f, cap, slots.get(), counts.get(), err, sizeof(err));
    EXPECT(rc == 0, "select bgr %dx%d: %s", H, W, err);
    rc = rh_crop_frames_host(table.data(), N, rows.data(), M, 0.3f, slots.get(), cap, &nm, out.get(), err, sizeof(err));
    EXPECT(rc == 0, "crop bgr %dx%d: %s", H, W, err);
    if (rc == 0) check_result("bgr", table.data(), N, rows, M, 0.3f, cap, slots.get(), counts.get(), out.get());
    for (int n = 0; n < N; ++n) EXPECT(blocks[n].same(), "bgr %dx%d: frame %d was written", H, W, n);
}

static void run_yuv(int H, int W, int N, int M, int cap)
{
    static const int BT601[6] = {1220542, 1673527, -852492, -409993, 2116026, 16}, BT709[6] = {1220542, 1880097, -558891, -223347, 2214593, 16};
    std::vector<Block> ys(N), cs(N);
    std::vector<RhYuvFrameDesc> table(N);
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    for (int n = 0; n < N; ++n) {
        const int form = rnd() % 3;
        RhYuvFrameDesc d;
        memset(&d, 0, sizeof(d));
        d.H = H; d.W = W; d.NH = H; d.NW = W; d.mid_off = -1;
        d.y_pix = 1; d.y_row = W + (rnd() % 2 ? 11 : 0);
        ys[n].alloc((size_t)((H - 1) * d.y_row + W));
        d.y_base = ys[n].buf.get();
        if (form < 2) {                                                                            // nv12 / nv21, pitched or not
            d.c_pix = 2; d.c_row = 2 * cw + (rnd() % 2 ? 10 : 0);
            cs[n].alloc((size_t)((ch - 1) * d.c_row + 2 * cw));
            d.u_base = cs[n].buf.get() + (form == 0 ? 0 : 1);
            d.v_base = cs[n].buf.get() + (form == 0 ? 1 : 0);
        } else {                                                                                   // i420: two planes in one block
            d.c_pix = 1; d.c_row = cw;
            cs[n].alloc((size_t)2 * ch * cw);
            d.u_base = cs[n].buf.get();
            d.v_base = cs[n].buf.get() + (size_t)ch * cw;
        }
        table[n] = d;
    }
    const std::vector<float> rows = fuzz_rows(N, M, H, W);
    std::unique_ptr<int[]> slots(new int[cap]), counts(new int[N]);
    std::unique_ptr<float[]> out(new float[(size_t)cap * 3 * RA_OUT_H * RA_OUT_W]);
    char err[256];
    const RaNorm nm = fuzz_norm();
    int rc = rh_select_host(table.data(), 1, N, rows.data(), M, 0.3f, cap, slots.get(), counts.get(), err, sizeof(err));
    EXPECT(rc == 0, "select yuv %dx%d: %s", H, W, err);
    rc = rh_crop_yuv_frames_host(table.data(), N, rnd() & 1 ? BT601 : BT709, rows.data(), M, 0.3f, slots.get(), cap, &nm, out.get(), err, sizeof(err));
    EXPECT(rc == 0, "crop yuv %dx%d: %s", H, W, err);
    if (rc == 0) check_result("yuv", table.data(), N, rows, M, 0.3f, cap, slots.get(), counts.get(), out.get());
    for (int n = 0; n < N; ++n) EXPECT(ys[n].same() && cs[n].same(), "yuv %dx%d: frame %d was written", H, W, n);
}

int main()
{
    static const int SIZES[][2] = {{1, 1}, {2, 2}, {7, 5}, {37, 53}, {64, 64}};
    for (int round = 0; round < 12; ++round)
        for (const auto& hw : SIZES) {
            const int N = 1 + rnd() % 3, M = rnd() % 9, cap = N + rnd() % 6;
            run_bgr(hw[0], hw[1], N, M, cap);
            run_yuv(hw[0], hw[1], N, M, cap);
        }
    // refusals: nothing is touched
    {
        char err[256];
        int slots[1] = {-7}, counts[2] = {-7, -7};
        RhFrameDesc t[2];
        memset(t, 0, sizeof(t));
        float row[RA_ROW] = {0};
        EXPECT(rh_select_host(t, 0, 2, row, 1, 0.3f, 1, slots, counts, err, sizeof(err)) == 1 && slots[0] == -7, "N > cap is refused");
        EXPECT(rh_select_host(t, 0, 1, row, 1, 0.3f, 0, slots, counts, err, sizeof(err)) == 1, "cap 0 is refused");
        RaNorm nm = {1.f, {0, 0, 0}, {1, 1, 1}, 0};
        float out[1];
        EXPECT(rh_crop_frames_host(t, 1, row, 1, 0.3f, slots, 1, &nm, out, err, sizeof(err)) == 1, "a null base is refused");
    }
    printf("reid_host_fuzz: %lld crops, %lld empty slots, %d failures\n", g_crops, g_empty, g_failures);
    return g_failures ? 1 : 0;
}
