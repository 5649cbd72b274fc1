// Host hygiene of the face-overlay host painters: csrc/face_draw_host.h (the bodies of cp_face_draw_frames_host and
// cp_face_draw_yuv_frames_host) compiled with the host compiler under AddressSanitizer + UBSan and run over seeded fuzz cases -- frame
// sizes 1x1, 2x2, 7x5, 37x53, 64x96; packed / 4-channel / padded BGR views and NV12 / I420 planes with pitches; landmarks, vertices and
// box corners in and far around the frame, +-1e9, +-3e38, NaN, +-inf, at the clamp; unused slots, invalid poses, cells outside the map
// handed over directly; every layer combination, radii 0..3, steps 1..9.  Every frame plane lives in a heap block of exactly its span
// (anything past it is the sanitizer's redzone: a store outside the frame is caught), every array in a block of exactly its size.
// Bytes no pixel channel addresses (a fourth channel, padding) must come back unchanged.
// CPU only:   make -C centerpose_amd/csrc face_draw_host_fuzz
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "face_draw_host.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }
static int g_failures = 0;
static long long g_changed = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { printf("FAIL: " __VA_ARGS__); printf("\n"); ++g_failures; } } while (0)
static const float SPECIAL[] = {1e9f, -1e9f, 3e38f, -3e38f, NAN, INFINITY, -INFINITY, 16384.f, -16384.f, 16383.5f};
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

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
};

static float coord(int extent) { return rnd() % 12 == 0 ? SPECIAL[rnd() % COUNT(SPECIAL)] : (float)uni(-extent - 8, 2 * extent + 8); }

static void run_case(int H, int W, int form)
{
    const int N = 1 + rnd() % 2, cap = N + rnd() % 4, V = 1 + rnd() % 300;
    const bool yuv = form >= 3;
    std::vector<Block> blocks(N * 3);
    std::vector<DrFrameDesc> bt(N);
    std::vector<DrYuvFrameDesc> yt(N);
    memset(bt.data(), 0, N * sizeof(DrFrameDesc));
    memset(yt.data(), 0, N * sizeof(DrYuvFrameDesc));
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
            if (form == 3) {
                Block& c = blocks[n * 3 + 1];
                c.alloc((size_t)((ch - 1) * 2 * cw + 2 * cw));
                yt[n].u_base = c.buf.get(); yt[n].v_base = c.buf.get() + 1; yt[n].c_row = 2 * cw; yt[n].c_pix = 2;
            } else {
                Block& u = blocks[n * 3 + 1];
                Block& v = blocks[n * 3 + 2];
                u.alloc((size_t)ch * cw); v.alloc((size_t)ch * cw);
                yt[n].u_base = u.buf.get(); yt[n].v_base = v.buf.get(); yt[n].c_row = cw; yt[n].c_pix = 1;
            }
        }
    }
    std::unique_ptr<int[]> slots(new int[cap]), box(new int[cap * 20]), valid(new int[cap]), ind(new int[V]);
    std::unique_ptr<float[]> lm(new float[(size_t)cap * FD_NKPT * 3]), pos(new float[(size_t)cap * FD_CELLS * 3]);
    for (int s = 0; s < cap; ++s) {
        slots[s] = rnd() % 4 == 0 ? -1 : (int)(rnd() % 1000);
        valid[s] = rnd() % 4 == 0 ? (int)(rnd() % 3) - 1 : 1;
        for (int i = 0; i < FD_NKPT * 3; ++i) lm[(size_t)s * FD_NKPT * 3 + i] = coord(i % 3 == 0 ? W : H);
        for (int i = 0; i < 20; ++i) box[s * 20 + i] = rnd() % 10 == 0 ? (rnd() % 2 ? -16384 : 16383) : (int)uni(-40, 2 * (i % 2 ? H : W) + 40);
        for (size_t i = 0; i < (size_t)FD_CELLS * 3; ++i) pos[(size_t)s * FD_CELLS * 3 + i] = 0.f;
    }
    for (int v = 0; v < V; ++v) {
        ind[v] = rnd() % 40 == 0 ? (rnd() % 2 ? FD_CELLS + (int)(rnd() % 4) : -1 - (int)(rnd() % 4)) : (int)(rnd() % FD_CELLS);
        if (ind[v] >= 0 && ind[v] < FD_CELLS)
            for (int s = 0; s < cap; ++s) {
                pos[((size_t)s * FD_CELLS + ind[v]) * 3] = coord(W);
                pos[((size_t)s * FD_CELLS + ind[v]) * 3 + 1] = coord(H);
            }
    }
    FdStyle st;
    memset(&st, 0, sizeof(st));
    st.landmarks = rnd() % 4 != 0; st.vertices = rnd() % 2; st.pose_box = rnd() % 2;
    st.landmark_radius = rnd() % 4; st.line_radius = rnd() % 4; st.box_radius = rnd() % 4; st.vertex_radius = rnd() % 4;
    st.vertex_step = 1 + rnd() % 9;
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 4; ++k) st.colors[c][k] = (unsigned char)rnd();
    const FdFaces f = {slots.get(), lm.get(), box.get(), valid.get(), pos.get(), ind.get(), V};
    char err[256];
    const int rc = yuv ? fd_draw_yuv_frames_host(yt.data(), N, cap, f, &st, err, sizeof(err)) : fd_draw_frames_host(bt.data(), N, cap, f, &st, err, sizeof(err));
    EXPECT(rc == 0, "refused: %s", err);
    for (int n = 0; n < N && !yuv && form != 0; ++n) {            // bytes no channel addresses keep their values
        const Block& b = blocks[n * 3];
        for (size_t i = 0; i < b.size; ++i) {
            const size_t in_row = i % (size_t)bt[n].row_stride;
            if (in_row >= (size_t)W * 4 || in_row % 4 == 3) EXPECT(b.buf[i] == b.orig[i], "form %d: byte %zu outside the pixels was written", form, i);
        }
    }
    for (const Block& b : blocks)
        for (size_t i = 0; i < b.size; ++i) g_changed += b.buf[i] != b.orig[i];
}

int main()
{
    static const int SIZES[][2] = {{1, 1}, {2, 2}, {7, 5}, {37, 53}, {64, 96}};
    int cases = 0;
    for (int rep = 0; rep < 6; ++rep)
        for (const auto& hw : SIZES)
            for (int form = 0; form < 5; ++form, ++cases) run_case(hw[0], hw[1], form);
    // refusals
    char err[256];
    int n[20] = {0};
    float x[4] = {0};
    DrFrameDesc d;
    memset(&d, 0, sizeof(d));
    FdStyle st;
    memset(&st, 0, sizeof(st));
    st.vertex_step = 1;
    FdFaces f = {n, x, nullptr, nullptr, nullptr, nullptr, 0};
    EXPECT(fd_draw_frames_host(&d, 1, 0, f, &st, err, sizeof(err)) == 1, "capacity 0 accepted");
    EXPECT(fd_draw_frames_host(&d, 2, 1, f, &st, err, sizeof(err)) == 1, "N > cap accepted");
    st.pose_box = 1;
    EXPECT(fd_draw_frames_host(&d, 1, 1, f, &st, err, sizeof(err)) == 1, "pose_box without a pose accepted");
    st.pose_box = 0; st.vertices = 1;
    EXPECT(fd_draw_frames_host(&d, 1, 1, f, &st, err, sizeof(err)) == 1, "vertices without maps accepted");
    st.vertices = 0; st.line_radius = 4;
    EXPECT(fd_draw_frames_host(&d, 1, 1, f, &st, err, sizeof(err)) == 1, "radius 4 accepted");
    st.line_radius = 1;
    EXPECT(fd_draw_frames_host(&d, 1, 1, f, &st, err, sizeof(err)) == 1, "null frame accepted");
    printf("face_draw_host_fuzz: %d cases, %lld bytes painted, %d failures\n", cases, g_changed, g_failures);
    return g_failures || g_changed == 0 ? 1 : 0;
}
