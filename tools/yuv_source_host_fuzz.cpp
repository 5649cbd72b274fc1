// Host hygiene of the shared YUV sampler: csrc/yuv_source.h (YsSource, ys_check_format, yf_yuv16_to_bgr) and the re-id YUV crop twin of
// csrc/reid_host.h on top of it, compiled with the host compiler under AddressSanitizer + UBSan and run over every format word the
// descriptor admits -- 4:2:0 / 4:2:2 / 4:4:4 / grey, 8-bit and 16-bit, semi-planar (interleaved pairs), planar and packed (YUYV / UYVY)
// layouts, pitched or not -- at sizes 1x1, 1x9, 9x1, 2x2, 7x5, 37x53, 64x64.  Every plane lives in a heap block of exactly the bytes
// its last sample ends at (anything past it is the sanitizer's redzone: one chroma sample too far, or a 16-bit load one byte too
// long, is a report); 16-bit blocks start at an address that is 2 but not 4 modulo 4.  Every pixel of every frame is loaded through
// both ys_source<true> and, for word 0, ys_source<false>, and compared with the conversion of the samples fetched by plain index
// arithmetic here; then the crop twin runs on fuzzed rows; frames must come back unchanged.  Refused words and alignments are tried.
// CPU only:   make -C centerpose_amd/csrc yuv_source_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "reid_host.h"

static uint64_t g_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static int g_failures = 0;
static long long g_pixels = 0, g_crops = 0;

#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            ++g_failures;                 \
        }                                 \
    } while (0)

// a heap block of exactly n bytes whose first byte lies at `lead` bytes past new[]'s (16-byte aligned) address: lead 2 puts 16-bit
// samples at 2 mod 4.  The lead bytes belong to the block, the n bytes end where the allocation ends.
struct Block {
    std::unique_ptr<unsigned char[]> buf, orig;
    size_t size = 0, lead = 0;
    void alloc(size_t n, size_t lead_)
    {
        size = n; lead = lead_;
        buf.reset(new unsigned char[n + lead]);
        orig.reset(new unsigned char[n + lead]);
        for (size_t i = 0; i < n + lead; ++i) buf[i] = orig[i] = (unsigned char)rnd();
    }
    unsigned char* p() const { return buf.get() + lead; }
    bool same() const { return memcmp(buf.get(), orig.get(), size + lead) == 0; }
};

struct FuzzFrame {
    Block y, c;
    RhYuvFrameDesc d;
};

static const int MATRICES[][6] = {{1220542, 1673527, -852492, -409993, 2116026, 16}, {1220542, 1880097, -558891, -223347, 2214593, 16},
                                  {1048576, 1470104, -748826, -360853, 1858077, 0},  {1048576, 1651297, -490864, -196424, 1945738, 0},
                                  {1220945, 1760217, -682019, -196426, 2245811, 16}, {1048576, 1546230, -599107, -172546, 1972791, 0}};

// layout 0: interleaved pairs (NV12-like: c_pix = 2 samples), 1: two planes in one block, 2: packed with the luma (YUYV / UYVY, 4:2:2 only)
static void make_frame(FuzzFrame& f, int H, int W, int fmt, int layout)
{
    const int b = (fmt & YS_16BIT) ? 2 : 1, sx = ys_sx(fmt), sy = ys_sy(fmt);
    const int ch = ((H - 1) >> sy) + 1, cw = ((W - 1) >> sx) + 1;
    RhYuvFrameDesc& d = f.d;
    memset(&d, 0, sizeof(d));
    d.H = H; d.W = W; d.NH = H; d.NW = W; d.mid_off = -1; d.pad = fmt;
    const size_t lead = b == 2 ? 2 : rnd() % 2;
    if (layout == 2) {                                             // W is even here: pixel pairs of 4 bytes (8 with 16-bit samples)
        const int uyvy = rnd() & 1;
        d.y_pix = 2 * b; d.y_row = (long long)W * 2 * b + (rnd() % 2 ? 6 * b : 0);
        d.c_pix = 2 * d.y_pix; d.c_row = d.y_row;
        f.y.alloc((size_t)((H - 1) * d.y_row + W * 2 * b), lead);
        d.y_base = f.y.p() + (uyvy ? b : 0);
        d.u_base = f.y.p() + (uyvy ? 0 : b);
        d.v_base = d.u_base + d.y_pix;
        f.c.alloc(0, 0);
        return;
    }
    d.y_pix = b; d.y_row = (long long)(W + (rnd() % 2 ? 11 : 0)) * b;
    f.y.alloc((size_t)((H - 1) * d.y_row + W * b), lead);
    d.y_base = f.y.p();
    if (fmt & YS_GREY) {
        f.c.alloc(0, 0);                                           // null chroma bases
        return;
    }
    if (layout == 0) {
        d.c_pix = 2 * b; d.c_row = (long long)(2 * cw + (rnd() % 2 ? 10 : 0)) * b;
        f.c.alloc((size_t)((ch - 1) * d.c_row + 2 * cw * b), lead);
        const int vu = rnd() & 1;
        d.u_base = f.c.p() + (vu ? b : 0);
        d.v_base = f.c.p() + (vu ? 0 : b);
    } else {
        d.c_pix = b; d.c_row = (long long)cw * b;
        f.c.alloc((size_t)2 * ch * cw * b, lead);
        d.u_base = f.c.p();
        d.v_base = f.c.p() + (size_t)ch * cw * b;
    }
}

static int sample(const unsigned char* base, long long off, int b)
{
    return b == 2 ? base[off] | (base[off + 1] << 8) : base[off];      // little-endian, by bytes
}

static void check_pixels(const FuzzFrame& f, const int* coef)
{
    const RhYuvFrameDesc& d = f.d;
    const YfCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    const int b = (d.pad & YS_16BIT) ? 2 : 1, sx = ys_sx(d.pad), sy = ys_sy(d.pad);
    const auto gen = ys_source<true>(d, k);
    const auto old = ys_source<false>(d, k);
    for (int r = 0; r < d.H; ++r)
        for (int c = 0; c < d.W; ++c) {
            const int Y = sample(d.y_base, r * d.y_row + c * d.y_pix, b);
            int U = b == 2 ? 32768 : 128, V = U;
            if (!(d.pad & YS_GREY)) {
                U = sample(d.u_base, (r >> sy) * d.c_row + (c >> sx) * d.c_pix, b);
                V = sample(d.v_base, (r >> sy) * d.c_row + (c >> sx) * d.c_pix, b);
            }
            int want[3], got[3];
            if (b == 2) yf_yuv16_to_bgr(Y, U, V, k, want); else yf_yuv_to_bgr(Y, U, V, k, want);
            gen.load(r, c, got);
            EXPECT(memcmp(want, got, sizeof(want)) == 0, "format %d, %d x %d, pixel (%d, %d): general sampler", d.pad, d.H, d.W, r, c);
            if (d.pad == 0) {
                old.load(r, c, got);
                EXPECT(memcmp(want, got, sizeof(want)) == 0, "format 0, %d x %d, pixel (%d, %d): 4:2:0 sampler", d.H, d.W, r, c);
            }
            for (int j = 0; j < 3; ++j) EXPECT(got[j] >= 0 && got[j] <= 255, "format %d: channel %d out of a byte", d.pad, got[j]);
            ++g_pixels;
        }
}

static std::vector<float> fuzz_rows(int M, int H, int W)
{
    static const float SPECIAL[] = {1e9f, -1e9f, 3e9f, NAN, INFINITY, -INFINITY};
    std::vector<float> rows((size_t)M * RA_ROW, 0.f);
    for (int m = 0; m < M; ++m) {
        float* row = &rows[(size_t)m * RA_ROW];
        const double cx = uni(-W, 2 * W), cy = uni(-H, 2 * H), w = uni(-2, W + 6), h = uni(-2, H + 6);
        row[0] = (float)(cx - w / 2); row[1] = (float)(cy - h / 2); row[2] = (float)(cx + w / 2); row[3] = (float)(cy + h / 2);
        if (rnd() % 6 == 0) row[rnd() % 4] = SPECIAL[rnd() % (sizeof(SPECIAL) / sizeof(SPECIAL[0]))];
        row[4] = rnd() % 4 ? 1.f : 0.3f;
    }
    rows[0] = 0.f; rows[1] = 0.f; rows[2] = (float)W; rows[3] = (float)H; rows[4] = 1.f;      // the whole frame: its last row and column are taps
    return rows;
}

static void check_crops(const FuzzFrame& f, const int* coef)
{
    const int M = 5, cap = 3;
    const std::vector<float> rows = fuzz_rows(M, f.d.H, f.d.W);
    std::unique_ptr<int[]> slots(new int[cap]), counts(new int[1]);
    std::unique_ptr<float[]> out(new float[(size_t)cap * 3 * RA_OUT_H * RA_OUT_W]);
    char err[256];
    const RaNorm nm = {1.f / 255.f, {0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, (int)(rnd() & 1)};
    int rc = rh_select_host(&f.d, 1, 1, rows.data(), M, 0.3f, cap, slots.get(), counts.get(), err, sizeof(err));
    EXPECT(rc == 0, "select, format %d: %s", f.d.pad, err);
    rc = rh_crop_yuv_frames_host(&f.d, 1, coef, rows.data(), M, 0.3f, slots.get(), cap, &nm, out.get(), err, sizeof(err));
    EXPECT(rc == 0, "crop, format %d, %d x %d: %s", f.d.pad, f.d.H, f.d.W, err);
    if (rc) return;
    for (int s = 0; s < cap; ++s) {
        bool finite = true;
        for (size_t i = 0; i < (size_t)3 * RA_OUT_H * RA_OUT_W; ++i) finite = finite && isfinite(out[(size_t)s * 3 * RA_OUT_H * RA_OUT_W + i]);
        EXPECT(finite, "format %d: slot %d holds a value that is not finite", f.d.pad, s);
        g_crops += slots[s] >= 0;
    }
}

int main()
{
    static const int SIZES[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {7, 5}, {37, 53}, {64, 64}};
    for (int round = 0; round < 3; ++round)
        for (const auto& hw : SIZES)
            for (int fmt = 0; fmt <= YS_FORMAT_MAX; ++fmt) {
                if (ys_check_word(fmt)) continue;
                for (int layout = 0; layout < 3; ++layout) {
                    if (layout == 2 && (ys_sx(fmt) != 1 || ys_sy(fmt) != 0 || (fmt & YS_GREY) || hw[1] % 2)) continue;
                    FuzzFrame f;
                    make_frame(f, hw[0], hw[1], fmt, layout);
                    const int* coef = MATRICES[rnd() % 6];
                    const char* bad = ys_check_format(f.d);
                    EXPECT(!bad, "format %d, layout %d, %d x %d is refused: %s", fmt, layout, hw[0], hw[1], bad ? bad : "");
                    if (bad) continue;
                    check_pixels(f, coef);
                    check_crops(f, coef);
                    EXPECT(f.y.same() && f.c.same(), "format %d, %d x %d: the frame was written", fmt, hw[0], hw[1]);
                }
            }
    // refusals: nothing is dereferenced
    {
        FuzzFrame f;
        make_frame(f, 4, 6, YS_16BIT, 0);
        RhYuvFrameDesc d = f.d;
        d.pad = 16; EXPECT(ys_check_format(d), "a format word of 16 is refused");
        d.pad = -1; EXPECT(ys_check_format(d), "a negative format word is refused");
        d.pad = YS_GREY | YS_FULL_X; EXPECT(ys_check_format(d), "grey with bit 0 is refused");
        d.pad = YS_GREY | YS_FULL_Y; EXPECT(ys_check_format(d), "grey with bit 1 is refused");
        d = f.d; d.y_base += 1; EXPECT(ys_check_format(d), "an odd luma base of 16-bit samples is refused");
        d = f.d; d.u_base += 1; EXPECT(ys_check_format(d), "an odd chroma base of 16-bit samples is refused");
        d = f.d; d.c_row += 1; EXPECT(ys_check_format(d), "an odd chroma stride of 16-bit samples is refused");
        d = f.d; d.y_pix = 3; EXPECT(ys_check_format(d), "an odd luma stride of 16-bit samples is refused");
        d = f.d; d.u_base = nullptr; EXPECT(ys_check_format(d), "a null chroma base is refused unless the frame is grey");
        d.pad = YS_GREY | YS_16BIT; d.v_base = nullptr; EXPECT(!ys_check_format(d), "a grey frame may have null chroma bases");
        char err[256];
        float row[RA_ROW] = {0, 0, 3, 3, 1.f};
        int slots[1] = {0};
        float out[1];
        const RaNorm nm = {1.f, {0, 0, 0}, {1, 1, 1}, 0};
        d = f.d; d.pad = 16;
        EXPECT(rh_crop_yuv_frames_host(&d, 1, MATRICES[0], row, 1, 0.3f, slots, 1, &nm, out, err, sizeof(err)) == 1, "the crop twin refuses word 16");
        int counts[1];
        EXPECT(rh_select_host(&d, 1, 1, row, 1, 0.3f, 1, slots, counts, err, sizeof(err)) == 1, "the selection refuses word 16");
    }
    // the 16-bit rule at its anchors: x << 8 gives the 8-bit rule's bytes; 10-bit studio black and white
    for (const auto& m : MATRICES) {
        const YfCoef k = {m[0], m[1], m[2], m[3], m[4], m[5]};
        for (int i = 0; i < 200000; ++i) {
            const int Y = rnd() & 255, U = rnd() & 255, V = rnd() & 255;
            int a[3], b[3];
            yf_yuv_to_bgr(Y, U, V, k, a);
            yf_yuv16_to_bgr(Y << 8, U << 8, V << 8, k, b);
            EXPECT(memcmp(a, b, sizeof(a)) == 0, "x << 8 differs from the 8-bit rule at (%d, %d, %d)", Y, U, V);
        }
    }
    {
        const YfCoef k = {MATRICES[0][0], MATRICES[0][1], MATRICES[0][2], MATRICES[0][3], MATRICES[0][4], MATRICES[0][5]};
        int p[3];
        yf_yuv16_to_bgr(64 << 6, 512 << 6, 512 << 6, k, p);
        EXPECT(p[0] == 0 && p[1] == 0 && p[2] == 0, "10-bit studio black");
        yf_yuv16_to_bgr(940 << 6, 512 << 6, 512 << 6, k, p);
        EXPECT(p[0] == 255 && p[1] == 255 && p[2] == 255, "10-bit studio white");
    }
    printf("yuv_source_host_fuzz: %lld pixels, %lld crops, %d failures\n", g_pixels, g_crops, g_failures);
    return g_failures ? 1 : 0;
}
