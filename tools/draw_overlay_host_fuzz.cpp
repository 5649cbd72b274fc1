// Host hygiene of the overlay host painters: csrc/draw_overlay_host.h (the bodies of cp_draw_overlay_frames_host and
// cp_draw_overlay_yuv_frames_host) and the score rule of csrc/draw_overlay_arith.h compiled with the host compiler under
// AddressSanitizer + UBSan and run over seeded fuzz cases -- frame sizes 1x1, 7x5, 16x16 (300 live rows), 37x53, 64x64; packed /
// 4-channel padded / planar BGR and RGB views; NV12 / NV21 / I420 planes, pitched, and a pitched surface; rows with coordinates far
// outside, +-1e9, NaN, +-inf, scores of both signs up to +-inf; labels at scales 1, 2 and 8 with prefixes of 0..9 glyphs, opacities
// 1..256, with and without row ids.  Every frame lives in a heap block of exactly its span plus guard bytes; after a call every byte
// that no view element addresses must be unchanged, and with opacities 256 and no labels the result must equal draw_host.h's.  The
// score rule is compared with printf's %.1f.  CPU only:   make -C centerpose_amd/csrc draw_overlay_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "draw_overlay_host.h"

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
static const float JSCORES[] = {1.f, 0.5f, 1e-30f, 0.f, -0.f, -1.f, NAN};
static const float RSCORES[] = {0.9f, 0.31f, 0.3f, 0.1f, NAN, 0.95f, 123.45f, 999.96f, INFINITY, 1e30f, 1.05f, 99.95f};

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
        row[4] = dense ? (float)uni(0.31, 1.2) : RSCORES[rnd() % 12];
        for (int j = 0; j < DA_JOINTS; ++j) {
            row[5 + 2 * j] = (float)(cx + uni(-w / 2 - 3, w / 2 + 3));
            row[6 + 2 * j] = (float)(cy + uni(-h / 2 - 3, h / 2 + 3));
            row[39 + j] = rnd() % 10 < 7 ? (float)uni(0.01, 1) : JSCORES[rnd() % 7];
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

static DoOverlay fuzz_overlay(int trial)
{
    static const int SC[] = {1, 2, 8, 0, 0, 3}, OP[] = {256, 128, 51, 1, 255, 256};
    DoOverlay ov;
    memset(&ov, 0xEE, sizeof(ov));                              // behind nprefix: glyph 0xEE, never read
    ov.label_scale = SC[trial % 6];
    for (int i = 0; i < 3; ++i) ov.opacity[i] = trial % 6 < 3 ? 256 : OP[rnd() % 6];
    ov.nprefix = trial % 2 ? (int)(rnd() % 10) : 6;
    for (int i = 0; i < ov.nprefix; ++i) ov.prefix[i] = (unsigned char)(rnd() % DT_GLYPHS);
    return ov;
}

static DaIdPalette fuzz_id_palette()
{
    DaIdPalette p;
    memset(&p, 0x11, sizeof(p));
    p.count = 1 + (int)(rnd() % DA_MAX_ID_COLORS);
    for (int i = 0; i < p.count; ++i)
        for (int k = 0; k < 4; ++k) p.colors[i][k] = (unsigned char)rnd();
    return p;
}

// form: 0 hwc bgr, 1 hwc bgra padded rows, 2 chw rgb 4 planes padded, 3 roi of a larger hwc rgb frame
static void bgr_frame(int form, int H, int W, Frame* f, DrFrameDesc* d)
{
    long long off = 0, row, pix, plane = 0;
    int C = 3;
    bool rgb = false, chw = false;
    switch (form) {
    case 0: row = 3 * W; pix = 3; break;
    case 1: row = 4 * W + 13; pix = 4; C = 4; break;
    case 2: row = W + 5; pix = 1; plane = (long long)H * (W + 5) + 9; C = 4; chw = true; rgb = true; break;
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

// form: 0 nv12 planes, 1 nv21 planes pitched, 2 i420 planes, 3 nv12 surface pitched (even sizes)
static void yuv_frame(int form, int H, int W, Frame* f, DrYuvFrameDesc* d)
{
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    long long y_row, u_off, v_off, c_row, c_pix;
    switch (form) {
    case 0: y_row = W; c_row = 2 * cw; c_pix = 2; u_off = (long long)H * W + 7; v_off = u_off + 1; break;
    case 1: y_row = W + 9; c_row = 2 * cw + 6; c_pix = 2; v_off = (long long)H * y_row + 3; u_off = v_off + 1; break;
    case 2: y_row = W; c_row = cw; c_pix = 1; u_off = (long long)H * W + 5; v_off = u_off + (long long)ch * cw + 5; break;
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

static void score_rule()
{
    static const char CH[] = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ #-.:_";
    int bad = 0, checked = 0;
    for (int i = 0; i < 300000; ++i) {
        union { float f; uint32_t u; } c;
        if (i % 3 == 0) c.u = rnd() * 2u + (rnd() & 1u);
        else c.f = (float)(i % 3 == 1 ? uni(0, 1.2) : uni(-999.9, 999.9));
        unsigned char g[8];
        memset(g, 0xEE, sizeof(g));
        const int n = do_score_glyphs(c.f, g);
        if (c.f != c.f) {
            bad += n != -1;
            continue;
        }
        bad += n < 3 || n > 6 || g[6] != 0xEE;
        if (n < 3 || n > 6 || !(fabsf(c.f) < 999.95f)) continue;
        char got[8] = {0}, want[32];
        for (int k = 0; k < n; ++k) got[k] = g[k] < DT_GLYPHS ? CH[g[k]] : '?';
        snprintf(want, sizeof(want), "%.1f", (double)c.f);
        bad += strcmp(got, want) != 0;
        ++checked;
    }
    EXPECT(bad == 0 && checked > 200000, "score rule: %d mismatches with %%.1f over %d values", bad, checked);
}

static void refusals()
{
    char err[256];
    DaStyle st = fuzz_style(0);
    DoOverlay ov = fuzz_overlay(0);
    DaIdPalette idp = fuzz_id_palette();
    float rows[2 * DA_ROW] = {0};
    int ids[2] = {0, 1};
    DrFrameDesc d;
    memset(&d, 0, sizeof(d));
    d.base = (unsigned char*)4096; d.row_stride = 24; d.pix_stride = 3; d.ch_off[1] = 1; d.ch_off[2] = 2; d.H = 4; d.W = 8;
    DrFrameDesc bad = d;
    bad.W = 0;
    EXPECT(do_draw_frames_host<false>(&bad, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &ov, err, sizeof(err)) == 1 && strstr(err, "bad size"),
           "W = 0 accepted: %s", err);
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, nullptr, nullptr, err, sizeof(err)) == 1 && strstr(err, "null overlay"),
           "null overlay accepted: %s", err);
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, ids, nullptr, &ov, err, sizeof(err)) == 1 && strstr(err, "together"),
           "row ids without a palette accepted: %s", err);
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, &idp, &ov, err, sizeof(err)) == 1 && strstr(err, "together"),
           "a palette without row ids accepted: %s", err);
    DoOverlay o = ov;
    o.opacity[1] = 0;
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &o, err, sizeof(err)) == 1 && strstr(err, "opacity"), "opacity 0");
    o = ov; o.opacity[2] = 257;
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &o, err, sizeof(err)) == 1 && strstr(err, "opacity"), "opacity 257");
    o = ov; o.label_scale = 9;
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &o, err, sizeof(err)) == 1 && strstr(err, "label_scale"), "scale 9");
    o = ov; o.nprefix = 10;
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &o, err, sizeof(err)) == 1 && strstr(err, "prefix"), "nprefix 10");
    o = ov; o.nprefix = 2; o.prefix[1] = DT_GLYPHS;
    EXPECT(do_draw_frames_host<false>(&d, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &o, err, sizeof(err)) == 1 && strstr(err, "glyph"), "glyph 42");
    EXPECT(do_draw_frames_host<false>(nullptr, 0, nullptr, 2, 0.3f, &st, nullptr, nullptr, &ov, err, sizeof(err)) == 0, "N = 0 refused");
    DrYuvFrameDesc y;
    memset(&y, 0, sizeof(y));
    y.y_base = (unsigned char*)4096; y.u_base = y.v_base = (unsigned char*)8192; y.y_row = 8; y.y_pix = 1; y.c_row = 8; y.c_pix = 2; y.H = 4; y.W = 8;
    EXPECT(do_draw_frames_host<true>(&y, 1, rows, 2, 0.3f, &st, nullptr, nullptr, &ov, err, sizeof(err)) == 1 && strstr(err, "one address"),
           "U == V accepted: %s", err);
}

template <bool YUV, int NF>
static void one_call(int H, int W, int M, int trial, int nforms, int* calls)
{
    typedef typename DrDesc<YUV>::type Desc;
    char err[256];
    const DaStyle st = fuzz_style(trial);
    const DoOverlay ov = fuzz_overlay(trial);
    const DaIdPalette idp = fuzz_id_palette();
    const bool with_ids = trial % 2 == 1;
    Frame f[NF], g[NF];
    Desc d[NF], e[NF];
    const uint64_t frames_state = g_state;
    for (int k = 0; k < nforms; ++k) {
        if constexpr (YUV) yuv_frame(k, H, W, &f[k], &d[k]);
        else bgr_frame(k, H, W, &f[k], &d[k]);
    }
    const std::vector<float> rows = fuzz_rows(nforms, M, H, W, M == 300);
    std::vector<int> ids((size_t)nforms * M);
    for (int& id : ids) id = rnd() % 3 == 0 ? -1 - (int)(rnd() % 5) : (int)(rnd() >> 1);
    const float vis = trial % 3 == 2 ? -1000.f : 0.3f;
    int rc = do_draw_frames_host<YUV>(d, nforms, rows.data(), M, vis, &st, with_ids ? ids.data() : nullptr, with_ids ? &idp : nullptr, &ov, err,
                                      sizeof(err));
    EXPECT(rc == 0, "%s %dx%d: rc %d: %s", YUV ? "yuv" : "bgr", H, W, rc, err);
    for (int k = 0; k < nforms; ++k) f[k].check(YUV ? "yuv" : "bgr");
    ++*calls;
    // the same frames once more (the same bytes: the generator is rewound), opaque and without labels, against draw_host.h's painter
    const uint64_t resume = g_state;
    for (int pass = 0; pass < 2; ++pass) {
        g_state = frames_state;
        for (int k = 0; k < nforms; ++k) {
            Frame* fr = pass ? &g[k] : &f[k];
            Desc* de = pass ? &e[k] : &d[k];
            if constexpr (YUV) yuv_frame(k, H, W, fr, de);
            else bgr_frame(k, H, W, fr, de);
        }
    }
    g_state = resume;
    DoOverlay plain = ov;
    plain.label_scale = 0;
    plain.opacity[0] = plain.opacity[1] = plain.opacity[2] = DO_OPAQUE;
    rc = do_draw_frames_host<YUV>(d, nforms, rows.data(), M, vis, &st, with_ids ? ids.data() : nullptr, with_ids ? &idp : nullptr, &plain, err,
                                  sizeof(err));
    EXPECT(rc == 0, "plain overlay: rc %d: %s", rc, err);
    if constexpr (YUV)
        rc = dr_draw_yuv_frames_host(e, nforms, rows.data(), M, vis, &st, err, sizeof(err), with_ids, ids.data(), &idp);
    else
        rc = dr_draw_frames_host(e, nforms, rows.data(), M, vis, &st, err, sizeof(err), with_ids, ids.data(), &idp);
    EXPECT(rc == 0, "plain painter: rc %d: %s", rc, err);
    for (int k = 0; k < nforms; ++k)
        EXPECT(f[k].size == g[k].size && memcmp(f[k].buf.get(), g[k].buf.get(), f[k].size) == 0, "%s %dx%d form %d: overlay at its defaults differs",
               YUV ? "yuv" : "bgr", H, W, k);
}

int main()
{
    static const int SIZES[][3] = {{1, 1, 12}, {7, 5, 12}, {16, 16, 300}, {37, 53, 12}, {64, 64, 12}};
    int calls = 0;
    for (const auto& sz : SIZES) {
        const int H = sz[0], W = sz[1], M = sz[2];
        for (int trial = 0; trial < 6; ++trial) {
            one_call<false, 4>(H, W, M, trial, 4, &calls);
            one_call<true, 4>(H, W, M, trial, (H % 2 == 0 && W % 2 == 0) ? 4 : 3, &calls);
        }
    }
    score_rule();
    refusals();
    EXPECT(g_painted > 0, "nothing was painted");
    printf("draw_overlay_host_fuzz: %d painter calls, %lld bytes painted, %d failures\n", calls, g_painted, g_failures);
    return g_failures ? 1 : 0;
}
