// Host hygiene of the heat-map host painters: csrc/draw_heat_host.h (the bodies of cp_draw_heat_frames_host and
// cp_draw_heat_yuv_frames_host) and the rule of csrc/draw_heat_arith.h compiled with the host compiler under AddressSanitizer + UBSan
// and run over seeded fuzz cases -- frame sizes 1x1, 7x5, 16x16, 37x53, 70x90; packed / 4-channel pitched / planar BGR and RGB views
// and crops at odd byte offsets; NV12 / NV21 / I420 planes with a pitch; maps of 1x1 .. 9x13 cells with 1..32 channels behind random
// element strides (batch views, permuted views) holding NaN, +-inf, huge and negative values; matrices that fit the frame, map it
// far outside the map on either side, collapse it onto one point or are as large as 1e308; every opacity class, invert on and off.
// Every frame and every map lives in a heap block of exactly its span (plus guard bytes for frames); after a call every byte that no
// view element addresses must be unchanged, and with opacity 256 a BGR pixel must hold exactly the sampled colour map.  The forward
// colour form is checked to stay inside a byte on all 2^24 colours.  CPU only:   make -C centerpose_amd/csrc draw_heat_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "draw_heat_host.h"

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

static const int SIZES[][2] = {{1, 1}, {7, 5}, {16, 16}, {37, 53}, {70, 90}};
static const float SPECIAL[] = {0.f, 1.f, 1.5f, -0.3f, NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e-40f, 254.999f / 255.f};

// maps of N x C x h x w values behind random element strides, in a heap block of exactly their span
struct Maps {
    std::unique_ptr<float[]> buf;
    long long stride[4];
    int N, C, h, w;
    void make(int N_, int C_, int h_, int w_)
    {
        N = N_; C = C_; h = h_; w = w_;
        const int extent[4] = {N, C, h, w};
        int order[4] = {0, 1, 2, 3};
        for (int i = 3; i > 0; --i) {
            const int j = rnd() % (i + 1), t = order[i];
            order[i] = order[j];
            order[j] = t;
        }
        long long span = 1;
        for (int i = 0; i < 4; ++i) {                          // innermost first in a random order of the dimensions, each behind a gap
            const int d = order[i];
            stride[d] = span + rnd() % 3;
            span += (extent[d] - 1) * stride[d];
        }
        if (rnd() % 5 == 0) stride[1] = 0;                     // an expanded channel dimension: the maps are only read, so allowed
        buf.reset(new float[(size_t)span]);
        for (long long i = 0; i < span; ++i) buf[i] = rnd() % 8 == 0 ? SPECIAL[rnd() % 11] : (float)pow(uni(0, 1), 3.0);
    }
};

static void fuzz_matrix(int trial, int H, int W, int h, int w, double* T)
{
    const double fit[6] = {(double)w / W * uni(0.8, 1.3), 0.0, uni(-1, 1), 0.0, (double)h / H * uni(0.8, 1.3), uni(-1, 1)};
    memcpy(T, fit, sizeof(fit));
    switch (trial % 7) {
    case 1: T[2] = 1e6; T[5] = -1e6; break;                    // the whole frame right of and above the map
    case 2: T[2] = -1e15; T[5] = 1e15; break;
    case 3: for (int i = 0; i < 6; ++i) T[i] = 0.0; break;     // every pixel onto cell (0, 0)
    case 4: T[0] = 1e308; T[1] = -1e308; T[4] = -1e308; T[3] = 1e308; break;      // overflow to +-inf, inf - inf = NaN inside the rule
    case 5: T[1] = uni(-0.5, 0.5); T[3] = uni(-0.5, 0.5); break;                   // sheared
    default: break;
    }
}

static DhStyle fuzz_style(int trial, int C)
{
    static const int OP[] = {179, 256, 1, 128, 255, 2};
    DhStyle s;
    memset(&s, 0xEE, sizeof(s));
    s.channels = trial % 2 ? C : C + (int)(rnd() % (unsigned)(DH_MAX_CHANNELS - C + 1));
    s.opacity = OP[trial % 6];
    s.invert = (trial / 3) % 2;
    for (int c = 0; c < s.channels; ++c)
        for (int k = 0; k < 4; ++k) s.palette[c][k] = (unsigned char)(rnd() % 4 == 0 ? (rnd() & 1 ? 255 : 0) : rnd());
    return s;
}

// a BGR / RGB frame of one of six forms -> its descriptor; marks the bytes its view addresses
static DrFrameDesc bgr_frame(Frame& f, int form, int H, int W)
{
    DrFrameDesc d;
    memset(&d, 0, sizeof(d));
    d.H = d.NH = H; d.W = d.NW = W; d.mid_off = -1;
    long long off = 0, chs = 1;
    int channels = 3;
    switch (form) {
    case 0: d.pix_stride = 3; d.row_stride = 3ll * W; break;                                        // packed
    case 1: d.pix_stride = 4; d.row_stride = 4ll * W; channels = 4; break;                          // 4 channels
    case 2: d.pix_stride = 4; d.row_stride = 4ll * W + 13; channels = 4; break;                     // pitched rows
    case 3: d.pix_stride = 1; d.row_stride = W; chs = (long long)H * W; break;                      // planar
    case 4: d.pix_stride = 1; d.row_stride = W + 5; chs = (long long)H * (W + 5) + 9; channels = 4; break;
    default: d.pix_stride = 3; d.row_stride = 3ll * (W + 9); off = (2ll * (W + 9) + 5) * 3 + form % 4; break;       // a crop, odd offsets
    }
    const bool rgb = rnd() & 1;
    for (int k = 0; k < 3; ++k) d.ch_off[k] = (rgb ? 2 - k : k) * chs;
    const long long span = off + (H - 1) * d.row_stride + (W - 1) * d.pix_stride + (channels - 1) * chs + 1;
    f.alloc((size_t)span);
    d.base = f.buf.get() + GUARD + off;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 3; ++k) f.mine[(size_t)(GUARD + off + y * d.row_stride + x * d.pix_stride + d.ch_off[k])] = 1;
    return d;
}

// a 4:2:0 frame: NV12 / NV21 (interleaved chroma) or I420 (two planes), with or without a pitch
static DrYuvFrameDesc yuv_frame(Frame& f, int form, int H, int W)
{
    DrYuvFrameDesc d;
    memset(&d, 0, sizeof(d));
    d.H = d.NH = H; d.W = d.NW = W; d.mid_off = -1;
    const int ch = (H + 1) / 2, cw = (W + 1) / 2, pitch = form & 1 ? 9 : 0;
    d.y_row = W + pitch; d.y_pix = 1;
    const long long ysz = (long long)H * d.y_row + 3;
    long long u_off, v_off, csz;
    if (form < 4) {                                            // nv12 (0, 1), nv21 (2, 3)
        d.c_pix = 2; d.c_row = 2ll * cw + (pitch ? 6 : 0);
        u_off = ysz + (form < 2 ? 0 : 1); v_off = ysz + (form < 2 ? 1 : 0);
        csz = (ch - 1) * d.c_row + (cw - 1) * 2 + 2;
    } else {                                                   // i420
        d.c_pix = 1; d.c_row = cw + (pitch ? 4 : 0);
        const long long plane = (ch - 1) * d.c_row + cw;
        u_off = ysz; v_off = ysz + plane + 5;
        csz = 2 * plane + 5;
    }
    f.alloc((size_t)(ysz + csz));
    unsigned char* b = f.buf.get() + GUARD;
    d.y_base = b; d.u_base = b + u_off; d.v_base = b + v_off;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            f.mine[(size_t)(GUARD + y * d.y_row + x)] = 1;
            const long long c = (y >> 1) * d.c_row + (x >> 1) * d.c_pix;
            f.mine[(size_t)(GUARD + u_off + c)] = f.mine[(size_t)(GUARD + v_off + c)] = 1;
        }
    return d;
}

int main()
{
    char err[256];
    // the forward form stays inside a byte, on every colour
    for (int matrix = 0; matrix < 2; ++matrix)
        for (int c = 0; c < (1 << 24); ++c) {
            int t[3];
            dh_bgr_to_yuv(c & 255, (c >> 8) & 255, c >> 16, matrix, t);
            if (t[0] < 0 || t[0] > 255 || t[1] < 0 || t[1] > 255 || t[2] < 0 || t[2] > 255) {
                EXPECT(false, "forward form %d leaves a byte at colour %06x", matrix, c);
                break;
            }
        }
    int calls = 0;
    for (int trial = 0; trial < 420; ++trial) {
        const int N = 1 + trial % 3, C = 1 + (int)(rnd() % DH_MAX_CHANNELS), h = 1 + (int)(rnd() % 9), w = 1 + (int)(rnd() % 13);
        Maps maps;
        maps.make(N, trial % 4 == 0 ? 1 : (trial % 4 == 1 ? 17 : C), h, w);
        const DhStyle st = fuzz_style(trial, maps.C);
        {
            std::vector<Frame> frames(N);
            std::vector<DrFrameDesc> table(N);
            for (int n = 0; n < N; ++n) {
                const int* sz = SIZES[(trial + n) % 5];
                table[n] = bgr_frame(frames[n], (trial + 2 * n) % 9, sz[0], sz[1]);
                fuzz_matrix(trial + n, sz[0], sz[1], h, w, table[n].mi);
            }
            const int rc = dh_draw_frames_host<false>(table.data(), N, maps.buf.get(), maps.stride, maps.C, h, w, &st, 0, err, sizeof(err));
            EXPECT(rc == 0, "trial %d: bgr painter refused: %s", trial, err);
            for (int n = 0; n < N; ++n) frames[n].check("bgr");
            if (st.opacity == DO_OPAQUE) {                     // the sampled colour map itself, whatever the frame held
                std::vector<uint32_t> cm((size_t)h * w);
                const DrFrameDesc& d = table[0];
                for (int i = 0; i < h; ++i)
                    for (int j = 0; j < w; ++j) cm[(size_t)i * w + j] = dh_cell(maps.buf.get() + i * maps.stride[2] + j * maps.stride[3], maps.stride[1], maps.C, st);
                size_t bad = 0;
                for (int y = 0; y < d.H; ++y)
                    for (int x = 0; x < d.W; ++x) {
                        int c[3];
                        dh_sample(cm.data(), h, w, d.mi, x, y, c);
                        for (int k = 0; k < 3; ++k) bad += d.base[y * d.row_stride + x * d.pix_stride + d.ch_off[k]] != c[k];
                    }
                EXPECT(bad == 0, "trial %d: %zu bytes differ from the sampled colour map at opacity 256", trial, bad);
            }
            ++calls;
        }
        {
            std::vector<Frame> frames(N);
            std::vector<DrYuvFrameDesc> table(N);
            for (int n = 0; n < N; ++n) {
                const int* sz = SIZES[(trial + n + 2) % 5];
                table[n] = yuv_frame(frames[n], (trial + n) % 6, sz[0], sz[1]);
                fuzz_matrix(trial + n + 3, sz[0], sz[1], h, w, table[n].mi);
            }
            const int rc = dh_draw_frames_host<true>(table.data(), N, maps.buf.get(), maps.stride, maps.C, h, w, &st, trial % 2, err, sizeof(err));
            EXPECT(rc == 0, "trial %d: yuv painter refused: %s", trial, err);
            for (int n = 0; n < N; ++n) frames[n].check("yuv");
            ++calls;
        }
    }
    // refusals touch nothing: a null table is never read when a check fails first
    {
        DhStyle st = fuzz_style(0, 2);
        const long long stride[4] = {48, 24, 6, 1}, neg[4] = {48, -1, 6, 1};
        float one = 0.f;
        EXPECT(dh_draw_frames_host<false>(nullptr, 1, &one, stride, 0, 4, 6, &st, 0, err, sizeof(err)) == 1, "C = 0 accepted");
        EXPECT(dh_draw_frames_host<false>(nullptr, 1, &one, stride, 33, 4, 6, &st, 0, err, sizeof(err)) == 1, "C = 33 accepted");
        EXPECT(dh_draw_frames_host<true>(nullptr, 1, &one, neg, 2, 4, 6, &st, 0, err, sizeof(err)) == 1, "a negative stride accepted");
        EXPECT(dh_draw_frames_host<true>(nullptr, 1, &one, stride, 2, 4, 6, &st, 2, err, sizeof(err)) == 1, "matrix id 2 accepted");
        EXPECT(dh_draw_frames_host<false>(nullptr, 1, &one, stride, 2, 4, 6, &st, 0, err, sizeof(err)) == 1, "a null table accepted");
        EXPECT(dh_draw_frames_host<false>(nullptr, 0, nullptr, stride, 2, 4, 6, &st, 0, err, sizeof(err)) == 0, "N = 0 refused");
        st.opacity = 0;
        EXPECT(dh_draw_frames_host<false>(nullptr, 0, nullptr, stride, 2, 4, 6, &st, 0, err, sizeof(err)) == 1, "opacity 0 accepted");
        DrFrameDesc d;
        memset(&d, 0, sizeof(d));
        unsigned char px[3] = {1, 2, 3};
        d.base = px; d.H = d.W = 1; d.ch_off[1] = 1; d.ch_off[2] = 2;
        d.mi[4] = NAN;
        st.opacity = 179;
        EXPECT(dh_draw_frames_host<false>(&d, 1, &one, stride, 1, 1, 1, &st, 0, err, sizeof(err)) == 1 && px[0] == 1, "a NaN matrix accepted");
    }
    EXPECT(g_painted > 100000, "only %lld bytes were painted", g_painted);
    printf("draw_heat_host_fuzz: %d painter calls, %lld bytes painted, %d failures\n", calls, g_painted, g_failures);
    return g_failures ? 1 : 0;
}
