// The aligned faces rendered on the device: a z-buffer rasteriser over every slot's position map -- the depth image, the per-pixel
// triangle index and the flat-shaded rendering that render_texture, get_triangle_buffer and get_depth_image compute per face in three
// nested Python loops after a download (demo/face/utils/render.py:85-120, 239-287; render_app.py:35-40), and the vertex colours of
// PRN.get_colors (demo/face/prnet.py:155-168).  The values are defined by face_render_arith.h (float64 on float32 inputs); the winner
// of a pixel is the maximum of one 64-bit key per covering triangle, so the result does not depend on the order in which the triangles
// arrive and is the same bits from run to run.
//
//   face_render_clear_kernel          : the key buffer [cap, h, w] to 0 ("no triangle"), a thread per key
//   face_render_raster_kernel         : grid (ceil(T / 256), cap), a thread per triangle.  The lane gathers its three vertices from the
//                                       map through face_ind (no vertex array exists), sets the triangle up and, where the box holds at
//                                       most 16 pixels (on a real face about one), walks it and issues a 64-bit atomicMax per covered
//                                       pixel.  A larger box goes to a list in LDS; after a barrier the block's 256 lanes walk each
//                                       listed box together, so a huge triangle costs its block box / 256 steps, not one lane the
//                                       whole window.  Unused slots exit at once.
//   face_render_resolve_kernel        : a thread per pixel: key -> tri, the winner's three attributes -> image
//   face_vertex_colors_kernel<..>     : grid (ceil(V / 256), cap), a thread per vertex: the frame's (B, G, R) at the vertex' cell,
//                                       through cp_frame_desc or cp_yuv_frame_desc (yuv_source.h; <surfaces> reads the format word)
//   cp_face_*_host                    : the sequential HOST twins of face_render_host.h, same statements
//
// The only atomics are the maxima on the keys (vector atomics, no return) and the LDS counter of the list; the list's order is the
// lanes' arrival order, which the maximum does not see.  Every write is to a pixel of the box, which fr_setup clamps to the window.
// The two tables (face_ind, tri) are the caller's to check when it uploads them: they are not re-checked per launch.
// Compiled with -ffp-contract=off.
#include "common.h"
#include "face_render_host.h"

#define FR_THREADS 256

template <bool YUV>
struct FrDesc { typedef RhFrameDesc type; };
template <>
struct FrDesc<true> { typedef RhYuvFrameDesc type; };

__global__ __launch_bounds__(FR_THREADS) void face_render_clear_kernel(unsigned long long* __restrict__ keys, int n)
{
    const int o = blockIdx.x * FR_THREADS + threadIdx.x;
    if (o < n) keys[o] = 0ull;
}

__device__ __forceinline__ void fr_vote(unsigned long long* keys, const FrTri& t, unsigned long long key, int x0, int y0, int w, int X, int Y)
{
    if (fr_covers(t, X, Y)) atomicMax(keys + (size_t)(Y - y0) * w + (X - x0), key);
}

__global__ __launch_bounds__(FR_THREADS) void face_render_raster_kernel(const float* __restrict__ pos, const int* __restrict__ slots,
                                                                        const int* __restrict__ face_ind, const int* __restrict__ tri, int T,
                                                                        const int* __restrict__ origin, int h, int w,
                                                                        unsigned long long* __restrict__ all_keys)
{
    __shared__ int big[FR_THREADS];
    __shared__ int nbig;
    const int s = blockIdx.y, l = threadIdx.x, i = blockIdx.x * FR_THREADS + l;
    if (!fr_slot_used(slots, origin, s)) return;                                // uniform over the block
    const float* map = pos + (size_t)s * FR_CELLS * 3;
    unsigned long long* keys = all_keys + (size_t)s * h * w;
    const int x0 = origin[2 * s], y0 = origin[2 * s + 1];
    if (l == 0) nbig = 0;
    __syncthreads();
    if (i < T) {
        const float* p[3];
        fr_gather(map, face_ind, tri, i, p);
        FrTri t;
        if (fr_setup(p[0], p[1], p[2], x0, y0, h, w, &t)) {
            const int bw = t.umax - t.umin + 1, bh = t.vmax - t.vmin + 1;      // <= 4096 each: the product fits an int
            if (bw * bh <= FR_LANE_BOX) {
                const unsigned long long key = fr_key(t.d, i);
                for (int Y = t.vmin; Y <= t.vmax; ++Y)
                    for (int X = t.umin; X <= t.umax; ++X) fr_vote(keys, t, key, x0, y0, w, X, Y);
            } else {
                big[atomicAdd(&nbig, 1)] = i;                                    // at most one entry per lane
            }
        }
    }
    __syncthreads();
    const int n = nbig;
    for (int e = 0; e < n; ++e) {
        const int j = big[e];
        const float* p[3];
        fr_gather(map, face_ind, tri, j, p);
        FrTri t;
        fr_setup(p[0], p[1], p[2], x0, y0, h, w, &t);                           // true: it was when the triangle was listed
        const unsigned long long key = fr_key(t.d, j);
        const int bw = t.umax - t.umin + 1, area = bw * (t.vmax - t.vmin + 1);
        for (int q = l; q < area; q += FR_THREADS) fr_vote(keys, t, key, x0, y0, w, t.umin + q % bw, t.vmin + q / bw);
    }
}

__global__ __launch_bounds__(FR_THREADS) void face_render_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                         const float* __restrict__ pos, const int* __restrict__ face_ind,
                                                                         const int* __restrict__ tri, const float* __restrict__ attrs, int V,
                                                                         int C, int window, int n, int* __restrict__ out_tri,
                                                                         float* __restrict__ out_image)
{
    const int o = blockIdx.x * FR_THREADS + threadIdx.x;
    if (o >= n) return;
    const int s = o / window;
    fr_resolve(keys[o], pos + (size_t)s * FR_CELLS * 3, face_ind, tri, attrs ? attrs + (size_t)s * V * C : nullptr, C, out_tri + o,
               out_image + (size_t)o * C);
}

template <bool YUV, bool GEN>
__global__ __launch_bounds__(FR_THREADS) void face_vertex_colors_kernel(const typename FrDesc<YUV>::type* __restrict__ table, int N,
                                                                        const float* __restrict__ pos, const int* __restrict__ slots, int cap,
                                                                        const int* __restrict__ face_ind, int V, YfCoef coef,
                                                                        float* __restrict__ colors)
{
    const int s = blockIdx.y, k = blockIdx.x * FR_THREADS + threadIdx.x, q = cap / N;
    if (k >= V) return;
    float r[3] = {0.f, 0.f, 0.f};
    if (slots[s] >= 0 && s / q < N) {                                           // uniform over the block
        const typename FrDesc<YUV>::type& d = table[s / q];
        const float* p = pos + ((size_t)s * FR_CELLS + face_ind[k]) * 3;
        if constexpr (YUV)
            fr_color(rh_yuv_source<GEN>(d, coef), d.H, d.W, p, r);
        else
            fr_color(rh_source(d), d.H, d.W, p, r);
    }
    float* o = colors + ((size_t)s * V + k) * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

#define FR_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" size_t cp_face_render_scratch_bytes(int cap, int h, int w, int T)
{
    char err[256];
    if (fr_check_sizes("face_render", cap, FR_MIN_V, T, h, w, err, sizeof(err))) return 0;
    return fr_scratch_bytes(cap, h, w);
}

extern "C" int cp_face_render_host(const float* pos, const int* slots, int cap, const int* face_ind, int V, const int* tri, int T,
                                   const int* origin, int h, int w, const float* attrs, int C, void* scratch, size_t scratch_bytes,
                                   int* out_tri, float* out_image)
{
    FR_FORWARD(fr_render_host(pos, slots, cap, face_ind, V, tri, T, origin, h, w, attrs, C, (uint64_t*)scratch, scratch_bytes, out_tri,
                              out_image, err, errn));
    return 0;
}

extern "C" int cp_face_vertex_colors_host(const void* table_host, int N, const float* pos, const int* slots, int cap, const int* face_ind,
                                          int V, float* colors)
{
    FR_FORWARD(fr_colors_host((const RhFrameDesc*)table_host, N, pos, slots, cap, face_ind, V, colors, err, errn));
    return 0;
}

extern "C" int cp_face_vertex_colors_yuv_host(const void* table_host, int N, const int* coef, const float* pos, const int* slots, int cap,
                                              const int* face_ind, int V, float* colors)
{
    FR_FORWARD(fr_colors_yuv_host((const RhYuvFrameDesc*)table_host, N, coef, pos, slots, cap, face_ind, V, colors, err, errn));
    return 0;
}

// face_ind DEVICE int [V] in 0..65535 and tri DEVICE int [T, 3] in 0..V-1: checked by the caller (face.FaceRenderer) when they are
// uploaded.  origin DEVICE int [cap, 2]: a slot whose origin lies outside +-2^20 is written like an unused one (fr_slot_used).
extern "C" int cp_face_render_f32(const float* pos, const int* slots, int cap, const int* face_ind, int V, const int* tri, int T,
                                  const int* origin, int h, int w, const float* attrs, int C, void* scratch, size_t scratch_bytes,
                                  int* out_tri, float* out_image, void* stream)
{
    const char* who = "face_render";
    FR_FORWARD(fr_check_call(who, cap, V, T, h, w, C, attrs != nullptr, scratch_bytes, err, errn));
    CP_CHECK_ARG(pos && slots && face_ind && tri && origin && scratch && out_tri && out_image, "%s: null pointer", who);
    CP_CHECK_ARG(((size_t)scratch & 7) == 0, "%s: the scratch is not 8-byte aligned", who);
    const int n = cap * h * w;                                                   // < 2^28 (fr_check_sizes)
    const unsigned pixel_blocks = (unsigned)((n + FR_THREADS - 1) / FR_THREADS);
    unsigned long long* keys = (unsigned long long*)scratch;
    hipLaunchKernelGGL(face_render_clear_kernel, dim3(pixel_blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, keys, n);
    CP_CHECK_LAUNCH("face_render_clear_kernel");
    hipLaunchKernelGGL(face_render_raster_kernel, dim3((unsigned)((T + FR_THREADS - 1) / FR_THREADS), (unsigned)cap), dim3(FR_THREADS), 0,
                       (hipStream_t)stream, pos, slots, face_ind, tri, T, origin, h, w, keys);
    CP_CHECK_LAUNCH("face_render_raster_kernel");
    hipLaunchKernelGGL(face_render_resolve_kernel, dim3(pixel_blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, keys, pos, face_ind, tri, attrs,
                       V, C, h * w, n, out_tri, out_image);
    CP_CHECK_LAUNCH("face_render_resolve_kernel");
    cp_note_kernel("face_render_clear_kernel+face_render_raster_kernel+face_render_resolve_kernel");
    return 0;
}

template <bool YUV>
static int fr_launch_colors(const char* who, const void* table, const void* table_host, int N, const int* coef, const float* pos,
                            const int* slots, int cap, const int* face_ind, int V, float* colors, void* stream)
{
    typedef typename FrDesc<YUV>::type Desc;
    FR_FORWARD(fr_check_colors(who, N, cap, V, err, errn));
    CP_CHECK_ARG(table && table_host && pos && slots && face_ind && colors, "%s: null pointer", who);
    YfCoef k = {0, 0, 0, 0, 0, 0};
    bool general = false;
    if constexpr (YUV) {
        FR_FORWARD(rh_check_yuv_frames(who, (const Desc*)table_host, N, coef, err, errn));
        k = YfCoef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
        for (int n = 0; n < N; ++n) general = general || ((const Desc*)table_host)[n].pad != 0;
    } else {
        FR_FORWARD(rh_check_frames(who, (const Desc*)table_host, N, err, errn));
    }
    const dim3 grid((unsigned)((V + FR_THREADS - 1) / FR_THREADS), (unsigned)cap);
    if (general)
        hipLaunchKernelGGL((face_vertex_colors_kernel<YUV, YUV>), grid, dim3(FR_THREADS), 0, (hipStream_t)stream, (const Desc*)table, N, pos,
                           slots, cap, face_ind, V, k, colors);
    else
        hipLaunchKernelGGL((face_vertex_colors_kernel<YUV, false>), grid, dim3(FR_THREADS), 0, (hipStream_t)stream, (const Desc*)table, N, pos,
                           slots, cap, face_ind, V, k, colors);
    CP_CHECK_LAUNCH("face_vertex_colors_kernel");
    cp_note_kernel(general ? "face_vertex_colors_kernel<surfaces>" : YUV ? "face_vertex_colors_kernel<yuv>" : "face_vertex_colors_kernel<bgr>");
    return 0;
}

extern "C" int cp_face_vertex_colors_f32(const void* table, const void* table_host, int N, const float* pos, const int* slots, int cap,
                                         const int* face_ind, int V, float* colors, void* stream)
{
    return fr_launch_colors<false>("face_vertex_colors", table, table_host, N, nullptr, pos, slots, cap, face_ind, V, colors, stream);
}

extern "C" int cp_face_vertex_colors_yuv_f32(const void* table, const void* table_host, int N, const int* coef, const float* pos,
                                             const int* slots, int cap, const int* face_ind, int V, float* colors, void* stream)
{
    return fr_launch_colors<true>("face_vertex_colors_yuv", table, table_host, N, coef, pos, slots, cap, face_ind, V, colors, stream);
}
