// Host hygiene of the draw_tracks host painters, the identity-coloured row painters and the per-row track ids: csrc/draw_tracks_host.h,
// csrc/draw_host.h and csrc/track_host.h (the bodies of cp_draw_tracks_*_host, cp_draw_rows_ids_*_host and cp_track_row_ids_host)
// compiled with the host compiler under AddressSanitizer + UBSan and run over seeded cases -- frame sizes 1x1, 7x5, 37x53, 64x96;
// packed / 4-channel padded BGR views and ROIs; NV12 / I420 planes, pitched; items far outside the frame, at the clamp limits and
// degenerate; labels of 0, 1 and 16 characters; scales 0..8, thickness 0..64; 300 items in one frame; counts that differ per frame.
// Every frame lives in a heap block of exactly its span plus guard bytes, the item table and the counts in blocks of exactly their
// size; after a call every byte that no view element addresses must be unchanged.  CPU only:
//     make -C centerpose_amd/csrc draw_tracks_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "draw_tracks_host.h"
#include "track_host.h"

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static int uni(int a, int b) { return a + (int)(rnd() % (uint32_t)(b - a + 1)); }      // a..b inclusive

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

// form: 0 hwc bgr, 1 hwc bgra with padded rows, 2 roi of a larger hwc rgb frame
static void bgr_frame(int form, int H, int W, Frame* f, DrFrameDesc* d)
{
    long long off = 0, row, pix;
    bool rgb = false;
    switch (form) {
    case 0: row = 3 * W; pix = 3; break;
    case 1: row = 4 * W + 13; pix = 4; break;
    default: row = (W + 11) * 3; pix = 3; off = (3 * (W + 11) + 4) * 3; rgb = true; break;
    }
    const long long span = off + (H - 1) * row + (W - 1) * pix + 3;
    f->alloc((size_t)span);
    memset(d, 0, sizeof(*d));
    d->base = f->buf.get() + GUARD + off;
    d->row_stride = row; d->pix_stride = pix;
    for (int k = 0; k < 3; ++k) d->ch_off[k] = rgb ? 2 - k : k;
    d->H = d->NH = H; d->W = d->NW = W; d->mid_off = -1;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 3; ++k) f->mine[GUARD + off + y * row + x * pix + k] = 1;
}

// form: 0 nv12 planes, 1 nv21 planes pitched, 2 i420 planes
static void yuv_frame(int form, int H, int W, Frame* f, DrYuvFrameDesc* d)
{
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    long long y_row, u_off, v_off, c_row, c_pix;
    switch (form) {
    case 0: y_row = W; c_row = 2 * cw; c_pix = 2; u_off = (long long)H * W + 7; v_off = u_off + 1; break;
    case 1: y_row = W + 9; c_row = 2 * cw + 6; c_pix = 2; v_off = (long long)H * y_row + 3; u_off = v_off + 1; break;
    default: y_row = W; c_row = cw; c_pix = 1; u_off = (long long)H * W + 5; v_off = u_off + (long long)ch * cw + 5; break;
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

static DtItem fuzz_item(int H, int W)
{
    DtItem it;
    memset(&it, 0xEE, sizeof(it));                  // the glyphs behind nchars hold an index outside the font: never read
    const int far = rnd() % 8;
    int ox = far == 0 ? -3 * W - 900 : (far == 1 ? 3 * W + 900 : 0), oy = far == 2 ? -3 * H - 900 : (far == 3 ? 3 * H + 900 : 0);
    if (far < 4 && (rnd() & 1)) { ox /= 40; oy /= 40; }
    it.x0 = uni(-8, W + 3) + ox; it.y0 = uni(-8, H + 3) + oy;
    it.x1 = it.x0 + (far == 4 ? 0 : uni(0, W + 7)); it.y1 = it.y0 + (far == 5 ? 0 : uni(0, H + 7));
    if (far == 6 && rnd() % 4 == 0) { it.x0 = it.y0 = -16384; it.x1 = it.y1 = 16383; }
    if (far == 7 && rnd() % 4 == 0) { it.x0 = it.x1 = 16383; it.y0 = it.y1 = 16383; }       // the bar's far corner: 16383 + 763
    static const int LENS[] = {0, 1, 16, 5};
    it.nchars = LENS[rnd() % 4];
    for (int c = 0; c < it.nchars; ++c) it.glyph[c] = (unsigned char)(rnd() % DT_GLYPHS);
    for (int k = 0; k < 4; ++k) { it.color[k] = (unsigned char)rnd(); it.text_color[k] = (unsigned char)rnd(); }
    return it;
}

// items[N][Kmax] and counts[N] in heap blocks of exactly their size
struct Items {
    std::unique_ptr<DtItem[]> items;
    std::unique_ptr<int[]> counts;
    int Kmax;
    Items(int N, int kmax, int H, int W, bool full) : items(new DtItem[(size_t)N * kmax]), counts(new int[N]), Kmax(kmax)
    {
        for (int n = 0; n < N; ++n) {
            counts[n] = full ? kmax : uni(0, kmax);
            for (int k = 0; k < kmax; ++k) {
                items[(size_t)n * kmax + k] = fuzz_item(H, W);
                if (k >= counts[n]) items[(size_t)n * kmax + k].nchars = 99;      // behind counts[n]: never looked at
            }
        }
    }
};

static void refusals()
{
    char err[256];
    DrFrameDesc d;
    memset(&d, 0, sizeof(d));
    d.base = (unsigned char*)4096; d.row_stride = 24; d.pix_stride = 3; d.ch_off[1] = 1; d.ch_off[2] = 2; d.H = 4; d.W = 8;
    DtItem it = fuzz_item(4, 8);
    it.nchars = 2; it.glyph[0] = 1; it.glyph[1] = 2;
    int count = 1;
    EXPECT(dk_draw_frames_host(&d, 1, &it, &count, 1, 65, 1, err, sizeof(err)) == 1 && strstr(err, "box_thickness"), "T = 65 accepted");
    EXPECT(dk_draw_frames_host(&d, 1, &it, &count, 1, 2, 9, err, sizeof(err)) == 1 && strstr(err, "font_scale"), "s = 9 accepted");
    EXPECT(dk_draw_frames_host(&d, 1, nullptr, &count, 1, 2, 1, err, sizeof(err)) == 1 && strstr(err, "null"), "null items accepted");
    EXPECT(dk_draw_frames_host(nullptr, 0, nullptr, nullptr, 1, 2, 1, err, sizeof(err)) == 0, "N = 0 refused");
    EXPECT(dk_draw_frames_host(&d, 1, nullptr, nullptr, 0, 2, 1, err, sizeof(err)) == 0, "Kmax = 0 refused");
    count = 2;
    EXPECT(dk_draw_frames_host(&d, 1, &it, &count, 1, 2, 1, err, sizeof(err)) == 1 && strstr(err, "Kmax"), "count > Kmax accepted");
    count = 1;
    it.glyph[1] = DT_GLYPHS;
    EXPECT(dk_draw_frames_host(&d, 1, &it, &count, 1, 2, 1, err, sizeof(err)) == 1 && strstr(err, "glyph"), "glyph 42 accepted");
    it.glyph[1] = 2; it.nchars = 17;
    EXPECT(dk_draw_frames_host(&d, 1, &it, &count, 1, 2, 1, err, sizeof(err)) == 1 && strstr(err, "characters"), "17 characters accepted");
    it.nchars = 2; it.x1 = it.x0 - 1;
    EXPECT(dk_draw_frames_host(&d, 1, &it, &count, 1, 2, 1, err, sizeof(err)) == 1 && strstr(err, "sorted"), "unsorted corners accepted");
    it.x1 = it.x0;
    DrFrameDesc bad = d;
    bad.W = 0;
    EXPECT(dk_draw_frames_host(&bad, 1, &it, &count, 1, 2, 1, err, sizeof(err)) == 1 && strstr(err, "bad size"), "W = 0 accepted: %s", err);
    // identity colours
    DaStyle st;
    memset(&st, 0, sizeof(st));
    st.box_thickness = 2; st.limb_radius = 1; st.joint_radius = 2;
    float rows[DA_ROW] = {0};
    int id = 3;
    DaIdPalette idp;
    memset(&idp, 0, sizeof(idp));
    EXPECT(dr_draw_frames_host(&d, 1, rows, 1, 0.3f, &st, err, sizeof(err), true, &id, &idp) == 1 && strstr(err, "id colours"), "count 0 accepted");
    idp.count = 65;
    EXPECT(dr_draw_frames_host(&d, 1, rows, 1, 0.3f, &st, err, sizeof(err), true, &id, &idp) == 1 && strstr(err, "id colours"), "count 65 accepted");
    idp.count = 1;
    EXPECT(dr_draw_frames_host(&d, 1, rows, 1, 0.3f, &st, err, sizeof(err), true, nullptr, &idp) == 1 && strstr(err, "row_ids"), "null ids accepted");
}

static void row_ids_cases()
{
    char err[256];
    static const int CASES[][4] = {{1, 1, 1, 1}, {2, 4, 9, 8}, {3, 5, 7, 17}, {2, 6, 4, 13}, {1, 3, 0, 3}};      // S, q, M, capacity
    for (const auto& c : CASES) {
        const int S = c[0], q = c[1], M = c[2], cap = c[3];
        std::unique_ptr<int[]> slots(new int[cap]), ids(new int[S * q]), out(new int[S * M > 0 ? S * M : 1]);
        for (int i = 0; i < cap; ++i) slots[i] = S * M > 0 ? uni(-1, S * M - 1) : -1;
        for (int i = 0; i < S * q; ++i) ids[i] = rnd() % 3 ? (int)(rnd() & 0x7fffffff) : -1;
        const int rc = th_row_ids_host(slots.get(), ids.get(), cap, S, q, M, out.get(), err, sizeof(err));
        EXPECT(rc == 0, "row ids %d %d %d %d: rc %d: %s", S, q, M, cap, rc, err);
        for (int r = 0; r < S * M; ++r) {
            int want = -1;
            for (int i = 0; i < S * q; ++i)
                if (slots[i] == r && ids[i] >= 0) want = ids[i];
            EXPECT(out[r] == want, "row ids: row %d holds %d, %d expected", r, out[r], want);
        }
        if (S * M > 0) {
            slots[S * q - 1] = S * M;
            EXPECT(th_row_ids_host(slots.get(), ids.get(), cap, S, q, M, out.get(), err, sizeof(err)) == 1 && strstr(err, "outside"), "slot S * M accepted");
        }
    }
}

int main()
{
    static const int SIZES[][3] = {{1, 1, 6}, {7, 5, 14}, {37, 53, 300}, {64, 96, 14}};
    char err[256];
    int calls = 0;
    for (const auto& sz : SIZES) {
        const int H = sz[0], W = sz[1], K = sz[2];
        for (int trial = 0; trial < 4; ++trial) {
            static const int TS[] = {3, 0, 64, 1}, SS[] = {2, 1, 8, 0};
            const int T = TS[trial], s = SS[trial];
            {   // the three BGR forms of this size in one call, each frame with its own items
                Frame f[3];
                DrFrameDesc d[3];
                for (int k = 0; k < 3; ++k) bgr_frame(k, H, W, &f[k], &d[k]);
                const Items it(3, K, H, W, trial == 0);
                const int rc = dk_draw_frames_host(d, 3, it.items.get(), it.counts.get(), K, T, s, err, sizeof(err));
                EXPECT(rc == 0, "bgr %dx%d: rc %d: %s", H, W, rc, err);
                for (int k = 0; k < 3; ++k) f[k].check("bgr");
                ++calls;
            }
            {
                Frame f[3];
                DrYuvFrameDesc d[3];
                for (int k = 0; k < 3; ++k) yuv_frame(k, H, W, &f[k], &d[k]);
                const Items it(3, K, H, W, trial == 0);
                const int rc = dk_draw_yuv_frames_host(d, 3, it.items.get(), it.counts.get(), K, T, s, err, sizeof(err));
                EXPECT(rc == 0, "yuv %dx%d: rc %d: %s", H, W, rc, err);
                for (int k = 0; k < 3; ++k) f[k].check("yuv");
                ++calls;
            }
            {   // identity-coloured rows: boxes and joints in the frame, ids of every kind, a palette block of exactly 260 bytes
                Frame f, g;
                DrFrameDesc d;
                DrYuvFrameDesc y;
                bgr_frame(trial % 3, H, W, &f, &d);
                yuv_frame(trial % 3, H, W, &g, &y);
                const int M = 9;
                std::unique_ptr<float[]> rows(new float[M * DA_ROW]);
                std::unique_ptr<int[]> ids(new int[M]);
                std::unique_ptr<DaIdPalette> idp(new DaIdPalette);
                memset(idp.get(), 0x5A, sizeof(DaIdPalette));
                idp->count = trial == 0 ? 1 : (trial == 1 ? 64 : 7);
                for (int m = 0; m < M; ++m) {
                    float* row = &rows[m * DA_ROW];
                    for (int k = 0; k < DA_ROW; ++k) row[k] = (float)uni(-6, (k % 2 ? H : W) + 6);
                    row[4] = 0.9f;
                    for (int j = 0; j < DA_JOINTS; ++j) row[39 + j] = rnd() % 4 ? 0.5f : 0.f;
                    static const int IDS[] = {-1, -7, 0, 5, 63, 64, 0x7fffffff};
                    ids[m] = IDS[rnd() % 7];
                }
                DaStyle st;
                memset(&st, 0x33, sizeof(st));
                st.box_thickness = 2; st.limb_radius = 1; st.joint_radius = 2;
                int rc = dr_draw_frames_host(&d, 1, rows.get(), M, 0.3f, &st, err, sizeof(err), true, ids.get(), idp.get());
                EXPECT(rc == 0, "ids bgr %dx%d: rc %d: %s", H, W, rc, err);
                rc = dr_draw_yuv_frames_host(&y, 1, rows.get(), M, 0.3f, &st, err, sizeof(err), true, ids.get(), idp.get());
                EXPECT(rc == 0, "ids yuv %dx%d: rc %d: %s", H, W, rc, err);
                f.check("ids bgr");
                g.check("ids yuv");
                calls += 2;
            }
        }
    }
    refusals();
    row_ids_cases();
    EXPECT(g_painted > 0, "nothing was painted");
    printf("draw_tracks_host_fuzz: %d painter calls, %lld bytes painted, %d failures\n", calls, g_painted, g_failures);
    return g_failures ? 1 : 0;
}
