// Host hygiene of the face-stage host twins: csrc/face_host.h (the bodies of cp_face_select_host, cp_face_crop_frames_host,
// cp_face_crop_yuv_frames_host and cp_face_restore_host) compiled with the host compiler under AddressSanitizer + UBSan and run over
// seeded fuzz cases -- frame sizes 1x1, 2x2, 7x5, 37x53, 64x64; packed / 4-channel / padded BGR views and NV12 / I420 planes with
// pitches; candidates (rows and boxes) far outside, reversed, empty, +-1e9, +-3e38, NaN, +-inf, scores at the threshold and NaN;
// capacities with and without spare slots; hostile slots / xform handed to the crop and the restore directly.  Every frame lives in a
// heap block of exactly its span (anything past it is the sanitizer's redzone: a tap outside the frame is caught), slots / counts /
// xform / out in blocks of exactly their size; frames must come back unchanged, an unused slot must be all zeros, every crop value
// must lie in 0..1 and no output may be NaN or infinite.
// CPU only:   make -C centerpose_amd/csrc face_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "face_host.h"

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

static const float SPECIAL[] = {1e9f, -1e9f, 3e38f, -3e38f, NAN, INFINITY, -INFINITY, 32768.f, -32768.f, 1e-30f};
static const float SCORES[] = {1.f, 0.5f, 0.3f, 0.30000004f, 1e-30f, 0.f, -1.f, NAN, INFINITY};
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

static std::vector<float> fuzz_cand(int N, int M, int H, int W, int boxes)
{
    const int stride = boxes ? FA_BOX : FA_ROW;
    std::vector<float> c((size_t)N * M * stride, 0.f);
    for (int r = 0; r < N * M; ++r) {
        float* row = &c[(size_t)r * stride];
        const double cx = uni(-W, 2 * W), cy = uni(-H, 2 * H), w = uni(-2, 2 * W + 6), h = uni(-2, 2 * H + 6);
        if (boxes) {
            row[0] = (float)(cx - w / 2); row[1] = (float)(cy - h / 2); row[2] = (float)(cx + w / 2); row[3] = (float)(cy + h / 2);
            if (rnd() % 5 == 0) row[rnd() % 4] = SPECIAL[rnd() % COUNT(SPECIAL)];
        } else {
            for (int j = 0; j < 5; ++j) {
                row[5 + 2 * j] = (float)(cx + uni(-w / 2, w / 2));
                row[6 + 2 * j] = (float)(cy + uni(-h / 2, h / 2));
            }
            if (rnd() % 5 == 0) row[5 + rnd() % 10] = SPECIAL[rnd() % COUNT(SPECIAL)];
        }
        row[4] = SCORES[rnd() % COUNT(SCORES)];
    }
    return c;
}

static void check_crops(const char* what, const int* slots, int cap, const float* out)
{
    const size_t crop = (size_t)3 * FA_RES * FA_RES;
    for (int s = 0; s < cap; ++s) {
        const float* o = out + (size_t)s * crop;
        bool any = false, ok = true;
        for (size_t i = 0; i < crop; ++i) {
            any = any || o[i] != 0.f;
            ok = ok && o[i] >= 0.f && o[i] <= 1.f;       // (NaN fails)
        }
        EXPECT(ok, "%s: slot %d holds a value outside 0..1", what, s);
        if (slots[s] < 0) EXPECT(!any, "%s: unused slot %d is not all zeros", what, s);
        if (any) ++g_crops; else ++g_empty;
    }
}

static void run_case(int H, int W, int form, int boxes)
{
    const int N = 1 + rnd() % 3, M = rnd() % 9, cap = N + rnd() % 5;
    const bool yuv = form >= 3;
    std::vector<Block> blocks(N * 3);
    std::vector<RhFrameDesc> bt(N);
    std::vector<RhYuvFrameDesc> yt(N);
    memset(bt.data(), 0, N * sizeof(RhFrameDesc));
    memset(yt.data(), 0, N * sizeof(RhYuvFrameDesc));
    for (int n = 0; n < N; ++n) {
        if (!yuv) {
            const int C = form == 0 ? 3 : 4;
            const long long row = (long long)W * C + (form == 2 ? 13 : 0);
            Block& b = blocks[n * 3];
            b.alloc((size_t)((H - 1) * row + (W - 1) * C + 3));
            bt[n].base = b.buf.get(); bt[n].row_stride = row; bt[n].pix_stride = C;
            bt[n].ch_off[0] = 0; bt[n].ch_off[1] = 1; bt[n].ch_off[2] = 2;
            bt[n].H = H; bt[n].W = W;
        } else {
            const int ch = (H + 1) / 2, cw = (W + 1) / 2;
            const long long yrow = W + (form == 4 ? 7 : 0);
            Block& y = blocks[n * 3];
            y.alloc((size_t)((H - 1) * yrow + W));
            yt[n].y_base = y.buf.get(); yt[n].y_row = yrow; yt[n].y_pix = 1; yt[n].H = H; yt[n].W = W;
            if (form == 3) {            // NV12: one interleaved chroma plane
                Block& c = blocks[n * 3 + 1];
                c.alloc((size_t)((ch - 1) * 2 * cw + 2 * cw));
                yt[n].u_base = c.buf.get(); yt[n].v_base = c.buf.get() + 1; yt[n].c_row = 2 * cw; yt[n].c_pix = 2;
            } else {                    // I420: two planes
                Block& u = blocks[n * 3 + 1];
                Block& v = blocks[n * 3 + 2];
                u.alloc((size_t)ch * cw); v.alloc((size_t)ch * cw);
                yt[n].u_base = u.buf.get(); yt[n].v_base = v.buf.get(); yt[n].c_row = cw; yt[n].c_pix = 1;
            }
        }
    }
    const std::vector<float> cand = fuzz_cand(N, M, H, W, boxes);
    std::unique_ptr<int[]> slots(new int[cap]), counts(new int[N]);
    std::unique_ptr<float[]> xform(new float[3 * cap]);
    const size_t crop = (size_t)3 * FA_RES * FA_RES;
    std::unique_ptr<float[]> out(new float[cap * crop]);
    char err[256];
    const FhRule rule = {0.3f, (rnd() % 4 == 0) ? (float)uni(0.01, 40) : 1.6f, 1 + (int)(rnd() % 3), boxes};
    int rc = fh_select_host(N, cand.data(), M, &rule, cap, slots.get(), counts.get(), xform.get(), err, sizeof(err));
    EXPECT(rc == 0, "select refused: %s", err);
    if (rc) return;
    const int q = cap / N;
    for (int s = 0; s < cap; ++s) {
        EXPECT(slots[s] == -1 || (s < N * q && slots[s] / M == s / q), "slot %d names candidate %d of another frame", s, slots[s]);
        EXPECT(isfinite(xform[3 * s + 2]) && (slots[s] < 0 ? xform[3 * s + 2] == 0.f : (xform[3 * s + 2] >= (float)rule.min_size && xform[3 * s + 2] <= 32768.f)),
               "slot %d: size %g", s, (double)xform[3 * s + 2]);
    }
    if (rnd() % 4 == 0 && cap > 0) {                                          // hostile values handed over directly
        const int s = rnd() % cap;
        slots[s] = (rnd() % 2) ? N * M + (int)(rnd() % 3) : (M ? (int)(rnd() % (N * M)) : -1);
        xform[3 * s] = SPECIAL[rnd() % COUNT(SPECIAL)];
        xform[3 * s + 1] = SPECIAL[rnd() % COUNT(SPECIAL)];
        xform[3 * s + 2] = (rnd() % 2) ? SPECIAL[rnd() % COUNT(SPECIAL)] : (float)uni(0, 40000);
    }
    const int coef[6] = {1220542, 1673527, -852492, -409993, 2116026, 16};
    rc = yuv ? fh_crop_yuv_frames_host(yt.data(), N, coef, M, slots.get(), xform.get(), cap, out.get(), err, sizeof(err))
             : fh_crop_frames_host(bt.data(), N, M, slots.get(), xform.get(), cap, out.get(), err, sizeof(err));
    EXPECT(rc == 0, "crop refused: %s", err);
    if (rc) return;
    check_crops(yuv ? "yuv" : "bgr", slots.get(), cap, out.get());
    for (const Block& b : blocks) EXPECT(b.size == 0 || b.same(), "a frame was written");

    // restore: the crop buffer stands in for the net's output (values in 0..1)
    int uv[2 * FA_NKPT];
    for (int i = 0; i < 2 * FA_NKPT; ++i) uv[i] = (i % 7 == 0) ? (i % 2 ? 255 : 0) : (int)(rnd() % FA_RES);
    const bool positions = rnd() % 2;
    std::unique_ptr<float[]> pos(positions ? new float[(size_t)cap * FA_RES * FA_RES * 3] : nullptr), lm(new float[(size_t)cap * FA_NKPT * 3]);
    rc = fh_restore_host(out.get(), slots.get(), xform.get(), cap, uv, pos.get(), lm.get(), err, sizeof(err));
    EXPECT(rc == 0, "restore refused: %s", err);
    for (int s = 0; s < cap && rc == 0; ++s)
        for (int j = 0; j < FA_NKPT; ++j) {
            const float* l = &lm[((size_t)s * FA_NKPT + j) * 3];
            FaXform t;
            const bool live = fh_slot(slots.get(), xform.get(), s, 1, FA_MAX_ROWS, &t);
            if (!live) EXPECT(l[0] == 0.f && l[1] == 0.f && l[2] == 0.f, "restore: unused slot %d has a landmark", s);
            if (live && isfinite(t.x0) && isfinite(t.y0)) EXPECT(isfinite(l[0]) && isfinite(l[1]) && isfinite(l[2]), "restore: slot %d landmark %d not finite", s, j);
            if (positions) {
                const float* p = &pos[(((size_t)s * FA_RES + uv[FA_NKPT + j]) * FA_RES + uv[j]) * 3];
                EXPECT(memcmp(p, l, 12) == 0, "restore: landmark %d of slot %d is not its cell", j, s);
            }
        }
}

int main()
{
    static const int SIZES[][2] = {{1, 1}, {2, 2}, {7, 5}, {37, 53}, {64, 64}};
    int cases = 0;
    for (int rep = 0; rep < 6; ++rep)
        for (const auto& hw : SIZES)
            for (int form = 0; form < 5; ++form)
                for (int boxes = 0; boxes < 2; ++boxes, ++cases) run_case(hw[0], hw[1], form, boxes);
    // refusals
    char err[256];
    int slots[2], counts[1];
    float xform[6];
    FhRule bad = {0.3f, 1.6f, 0, 0};
    EXPECT(fh_select_host(1, nullptr, 0, &bad, 2, slots, counts, xform, err, sizeof(err)) == 1, "min_size 0 accepted");
    bad.min_size = 1; bad.expand = NAN;
    EXPECT(fh_select_host(1, nullptr, 0, &bad, 2, slots, counts, xform, err, sizeof(err)) == 1, "NaN expand accepted");
    bad.expand = 1.6f;
    EXPECT(fh_select_host(3, nullptr, 0, &bad, 2, slots, counts, xform, err, sizeof(err)) == 1, "N > cap accepted");
    EXPECT(fh_select_host(1, nullptr, 0, &bad, 2, slots, counts, xform, err, sizeof(err)) == 0 && slots[0] == -1 && slots[1] == -1 && counts[0] == 0,
           "M = 0 refused");
    printf("face_host_fuzz: %d cases, %lld crops with pixels, %lld empty, %d failures\n", cases, g_crops, g_empty, g_failures);
    return g_failures ? 1 : 0;
}
