// Host hygiene of the draw_results host painters: csrc/draw_host.h (the bodies of cp_draw_rows_frames_host and
// cp_draw_rows_yuv_frames_host) compiled with the host compiler under AddressSanitizer + UBSan and run over seeded fuzz cases --
// frame sizes 1x1, 7x5, 16x16 (300 live rows), 37x53, 64x64; packed / planar / 4-channel / padded / ROI BGR and RGB views; NV12 /
// NV21 / I420 planes, pitched, interleaved chroma views, surfaces; rows with coordinates far outside, +-1e9, NaN, +-inf, scores at
// the threshold and NaN.  Every frame lives in a heap block of exactly its span plus guard bytes; after a call every byte that no
// view element addresses must be unchanged.  CPU only:   make -C centerpose_amd/csrc draw_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "draw_host.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static const int GUARD = 64;
static int g_failures = 0;
static long long g_painted = 0;

#define EXPECT(cond, ...)                \
    do {                                 \
        if (!(cond)) {                   \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                \
            ++g_failures;                \
        }                                \
    } while (0)

struct Frame {
    std::unique_ptr<unsigned char[]> buf, orig;     // exactly `size` bytes: anything past them is the sanitizer's redzone
    std::vector<char> mine;                         // bytes a view element addresses
    size_t size = 0;
    void alloc(size_t n)
    {
        size = n + 2 * GUARD;
        buf.reset(new unsigned char[size]);
        orig.reset(new unsigned char[size]);
        for (size_t i = 0; i < size; ++i) buf[i] = orig[i] = (unsigned char)rnd();
        mine.assign(size, 0);
    }
    void check(const char* what)
    {
        size_t bad = 0;
        for (size_t i = 0; i < size; ++i) {
            if (!mine[i] && buf[i] != orig[i]) ++bad;
            if (buf[i] != orig[i]) ++g_painted;
        }
        EXPECT(bad == 0, "%s: %zu bytes outside the view were written", what, bad);
    }
};

static const float SPECIAL[] = {1e9f, -1e9f, NAN, INFINITY, -INFINITY, 16383.9f, -16384.9f, 20000.f, -20000.f};
static const float SCORES[] = {1.f, 0.5f, 1e-30f, 0.f, -0.f, -1.f, NAN};

static std::vector<float> fuzz_rows(int N, int M, int H, int W, bool dense)
{
    std::vector<float> rows((size_t)N * M * DA_ROW, 0.f);
    for (int r = 0; r < N * M; ++r) {
        float* row = &rows[(size_t)r * DA_ROW];
        const int far = rnd() % 6;
        double ox = far == 0 ? -3.0 * W - 40 : (far == 1 ? 3.0 * W + 40 : 0), oy = far == 2 ? -3.0 * H - 40 : (far == 3 ? 3.0 * H + 40 : 0);
        if (far < 4 && (rnd() & 1)) { ox /= 3; oy /= 3; }
        const double cx = uni(-4, W + 4) + ox, cy = uni(-4, H + 4) + oy, w = uni(0, W + 6), h = uni(0, H + 6);
        const bool rev = rnd() % 3 == 0;
        row[rev ? 2 : 0] = (float)(cx - w / 2); row[rev ? 3 : 1] = (float)(cy - h / 2);
        row[rev ? 0 : 2] = (float)(cx + w / 2); row[rev ? 1 : 3] = (float)(cy + h / 2);
        const float scores[] = {0.9f, 0.31f, 0.3f, 0.1f, NAN, 0.9f};
        row[4] = dense ? 1.f : scores[rnd() % 6];
        for (int j = 0; j < DA_JOINTS; ++j) {
            row[5 + 2 * j] = (float)(cx + uni(-w / 2 - 3, w / 2 + 3));
            row[6 + 2 * j] = (float)(cy + uni(-h / 2 - 3, h / 2 + 3));
            row[39 + j] = rnd() % 10 < 7 ? (float)uni(0.01, 1) : SCORES[rnd() % 7];
        }
        for (int k = rnd() % 4; k > 0; --k) {
            int at = rnd() % 38;
            at = at < 4 ? at : at + 1;                         // a box or joint coordinate, not the score
            row[at] = SPECIAL[rnd() % 9];
        }
    }
    return rows;
}

static DaStyle fuzz_style(int trial)
{
    static const int TS[] = {0, 1, 2, 3, 5, 64}, LS[] = {-1, 1, 2, 3, 4, 64}, JS[] = {-1, 0, 1, 2, 3, 6, 64};
    DaStyle s;
    s.box_thickness = trial % 3 == 0 ? 2 : TS[rnd() % 6];
    s.limb_radius = trial % 3 == 0 ? 1 : LS[rnd() % 6];
    s.joint_radius = trial % 3 == 0 ? 2 : JS[rnd() % 7];
    for (int l = 0; l < DA_PRIMS; ++l)
        for (int k = 0; k < 4; ++k) s.palette[l][k] = (unsigned char)rnd();
    return s;
}

// form: 0 hwc bgr, 1 hwc rgb 4ch, 2 hwc bgra padded rows, 3 chw rgb, 4 chw 4 planes padded, 5 roi of a larger hwc rgb frame
static void bgr_frame(int form, int H, int W, Frame* f, DrFrameDesc* d)
{
    long long off = 0, row, pix, plane = 0;
    int C = 3;
    bool rgb = false, chw = false;
    switch (form) {
    case 0: row = 3 * W; pix = 3; break;
    case 1: row = 4 * W; pix = 4; C = 4; rgb = true; break;
    case 2: row = 4 * W + 13; pix = 4; C = 4; break;
    case 3: row = W; pix = 1; plane = (long long)H * W; rgb = true; chw = true; break;
    case 4: row = W + 5; pix = 1; plane = (long long)H * (W + 5) + 9; C = 4; chw = true; break;
    default: row = (W + 11) * 3; pix = 3; off = (3 * (W + 11) + 4) * 3; rgb = true; break;
    }
    const long long cs = chw ? plane : 1;
    const long long span = off + (H - 1) * row + (W - 1) * pix + (C - 1) * cs + 1;
    f->alloc((size_t)span);
    memset(d, 0, sizeof(*d));
    d->base = f->buf.get() + GUARD + off;
    d->row_stride = row; d->pix_stride = pix;
    for (int k = 0; k < 3; ++k) d->ch_off[k] = (rgb ? 2 - k : k) * cs;
    d->H = d->NH = H; d->W = d->NW = W; d->mid_off = -1;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 3; ++k) f->mine[GUARD + off + y * row + x * pix + k * cs] = 1;
}

// form: 0 nv12 planes, 1 nv21 planes pitched, 2 i420 planes, 3 i420 with interleaved chroma views, 4 nv12 surface pitched (even sizes)
static void yuv_frame(int form, int H, int W, Frame* f, DrYuvFrameDesc* d)
{
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    long long y_row, u_off, v_off, c_row, c_pix;
    switch (form) {
    case 0: y_row = W; c_row = 2 * cw; c_pix = 2; u_off = (long long)H * W + 7; v_off = u_off + 1; break;
    case 1: y_row = W + 9; c_row = 2 * cw + 6; c_pix = 2; v_off = (long long)H * y_row + 3; u_off = v_off + 1; break;
    case 2: y_row = W; c_row = cw; c_pix = 1; u_off = (long long)H * W + 5; v_off = u_off + (long long)ch * cw + 5; break;
    case 3: y_row = W + 3; c_row = 2 * cw; c_pix = 2; u_off = (long long)H * y_row + 2; v_off = u_off + 1; break;
    default: y_row = W + 16; c_row = y_row; c_pix = 2; u_off = (long long)H * y_row; v_off = u_off + 1; break;
    }
    const long long c_last = (ch - 1) * c_row + (cw - 1) * c_pix;
    const long long span = (u_off > v_off ? u_off : v_off) + c_last + 1;
    f->alloc((size_t)span);
    memset(d, 0, sizeof(*d));
    d->y_base = f->buf.get() + GUARD; d->y_row = y_row; d->y_pix = 1;
    d->u_base = d->y_base + u_off; d->v_base = d->y_base + v_off; d->c_row = c_row; d->c_pix = c_pix;
    d->H = d->NH = H; d->W = d->NW = W; d->mid_off = -1;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) f->mine[GUARD + y * y_row + x] = 1;
    for (int y = 0; y < ch; ++y)
        for (int x = 0; x < cw; ++x) f->mine[GUARD + u_off + y * c_row + x * c_pix] = f->mine[GUARD + v_off + y * c_row + x * c_pix] = 1;
}

static void refusals()
{
    char err[256];
    DaStyle st = fuzz_style(0);
    float rows[2 * DA_ROW] = {0};
    DrFrameDesc d;
    memset(&d, 0, sizeof(d));
    d.base = (unsigned char*)4096; d.row_stride = 24; d.pix_stride = 3; d.ch_off[1] = 1; d.ch_off[2] = 2; d.H = 4; d.W = 8;
    DrFrameDesc bad = d;
    bad.W = 0;
    EXPECT(dr_draw_frames_host(&bad, 1, rows, 2, 0.3f, &st, err, sizeof(err)) == 1 && strstr(err, "bad size"), "W = 0 accepted: %s", err);
    bad = d; bad.pix_stride = 0;
    EXPECT(dr_draw_frames_host(&bad, 1, rows, 2, 0.3f, &st, err, sizeof(err)) == 1 && strstr(err, "stride of 0"), "stride 0 accepted: %s", err);
    EXPECT(dr_draw_frames_host(&d, 1, rows, 2, NAN, &st, err, sizeof(err)) == 1, "NaN threshold accepted");
    EXPECT(dr_draw_frames_host(&d, 1, nullptr, 2, 0.3f, &st, err, sizeof(err)) == 1, "null rows accepted");
    EXPECT(dr_draw_frames_host(nullptr, 0, nullptr, 2, 0.3f, &st, err, sizeof(err)) == 0, "N = 0 refused");
    EXPECT(dr_draw_frames_host(&d, 1, nullptr, 0, 0.3f, &st, err, sizeof(err)) == 0, "M = 0 refused");
    st.limb_radius = 0;
    EXPECT(dr_draw_frames_host(&d, 1, rows, 2, 0.3f, &st, err, sizeof(err)) == 1 && strstr(err, "limb_radius"), "limb radius 0 accepted");
    DrYuvFrameDesc y;
    memset(&y, 0, sizeof(y));
    y.y_base = (unsigned char*)4096; y.u_base = y.v_base = (unsigned char*)8192; y.y_row = 8; y.y_pix = 1; y.c_row = 8; y.c_pix = 2; y.H = 4; y.W = 8;
    st.limb_radius = 1;
    EXPECT(dr_draw_yuv_frames_host(&y, 1, rows, 2, 0.3f, &st, err, sizeof(err)) == 1 && strstr(err, "one address"), "U == V accepted: %s", err);
}

int main()
{
    static const int SIZES[][3] = {{1, 1, 12}, {7, 5, 12}, {16, 16, 300}, {37, 53, 12}, {64, 64, 12}};
    char err[256];
    int calls = 0;
    for (const auto& sz : SIZES) {
        const int H = sz[0], W = sz[1], M = sz[2];
        for (int trial = 0; trial < 3; ++trial) {
            const DaStyle st = fuzz_style(trial);
            {   // all six BGR forms of this size in one call, each frame with its own rows
                Frame f[6];
                DrFrameDesc d[6];
                for (int k = 0; k < 6; ++k) bgr_frame(k, H, W, &f[k], &d[k]);
                const std::vector<float> rows = fuzz_rows(6, M, H, W, M == 300);
                const int rc = dr_draw_frames_host(d, 6, rows.data(), M, 0.3f, &st, err, sizeof(err));
                EXPECT(rc == 0, "bgr %dx%d: rc %d: %s", H, W, rc, err);
                for (int k = 0; k < 6; ++k) f[k].check("bgr");
                ++calls;
            }
            {
                const int n = (H % 2 == 0 && W % 2 == 0) ? 5 : 4;
                Frame f[5];
                DrYuvFrameDesc d[5];
                for (int k = 0; k < n; ++k) yuv_frame(k, H, W, &f[k], &d[k]);
                const std::vector<float> rows = fuzz_rows(n, M, H, W, M == 300);
                const int rc = dr_draw_yuv_frames_host(d, n, rows.data(), M, 0.3f, &st, err, sizeof(err));
                EXPECT(rc == 0, "yuv %dx%d: rc %d: %s", H, W, rc, err);
                for (int k = 0; k < n; ++k) f[k].check("yuv");
                ++calls;
            }
        }
    }
    refusals();
    EXPECT(g_painted > 0, "nothing was painted");
    printf("draw_host_fuzz: %d painter calls, %lld bytes painted, %d failures\n", calls, g_painted, g_failures);
    return g_failures ? 1 : 0;
}
