// The face overlays on device frames, in place: the 68 landmarks with their connecting lines (plot_kpt), the dense vertices
// (plot_vertices) and the pose box (plot_pose_box) of demo/face/utils/cv_plot.py for every face of every frame, from the FaceResult
// where it lies on the device.  The picture is defined by face_draw_arith.h; the frames are addressed by the descriptors of
// draw_results (cp_frame_desc: packed / planar BGR or RGB, 3 or 4 channels, any strides; cp_yuv_frame_desc: 8-bit 4:2:0).
//
//   face_draw_build_kernel         : grid cap, 256 threads.  Thread i builds primitive i of its slot's face; the block writes the
//                                    face's header (bounding box, mask of existing primitives); an unused slot gets an empty header.
//   face_draw_vertices_kernel<bgr|yuv> : grid (ceil(drawn vertices / 256), cap), one thread per drawn vertex: a scatter of clipped
//                                    discs.  Launched first: the vertices lie beneath everything else.  Every store writes the same
//                                    bytes, so the result does not depend on the order of the threads.
//   face_draw_kernel<bgr|yuv>      : one block per 16 x 16 pixel tile and frame (YUV: 32 x 32 pixels, a 2 x 2 block per thread).  A
//                                    thread walks its frame's faces from the back, rejects a face by its bounding box, and stores the
//                                    colour of the last covering primitive: three bytes per covered pixel (YUV: luma per pixel,
//                                    chroma from the latest-painted colour among the sample's pixels).
//   cp_face_draw_*_host            : the sequential HOST painters of face_draw_host.h, same statements
#include "common.h"
#include "face_draw_host.h"

#define FD_THREADS 256
#define FD_TILE 16

__global__ __launch_bounds__(FD_THREADS) void face_draw_build_kernel(FdFaces f, FdStyle st, FdHeader* __restrict__ hdr,
                                                                     DaPrim* __restrict__ prims)
{
    __shared__ int bb[4];
    __shared__ unsigned long long mask[3];
    const int s = blockIdx.x, i = threadIdx.x;
    if (i == 0) { bb[0] = INT32_MAX; bb[1] = INT32_MAX; bb[2] = INT32_MIN; bb[3] = INT32_MIN; }
    if (i < 3) mask[i] = 0ull;
    __syncthreads();
    if (i < FD_PRIMS && f.slots[s] >= 0) {
        DaPrim p;
        if (fd_build(f.landmarks + (size_t)s * FD_NKPT * 3, f.box ? f.box + (size_t)s * 20 : nullptr, f.valid ? f.valid[s] : 0, st, i, &p)) {
            int x0, y0, x1, y1;
            da_bounds(p, fd_radius(st, i), &x0, &y0, &x1, &y1);
            prims[(size_t)s * FD_STRIDE + i] = p;
            atomicMin(&bb[0], x0); atomicMin(&bb[1], y0); atomicMax(&bb[2], x1); atomicMax(&bb[3], y1);
            atomicOr(&mask[i >> 6], 1ull << (i & 63));
        }
    }
    __syncthreads();
    if (i == 0) hdr[s] = FdHeader{bb[0], bb[1], bb[2], bb[3], {mask[0], mask[1], mask[2]}, 0ull};
}

template <bool YUV>
__device__ inline void fd_store(const typename DrDesc<YUV>::type& d, int x, int y, const unsigned char* col)
{
    if constexpr (YUV) {
        const long long c = (long long)(y >> 1) * d.c_row + (long long)(x >> 1) * d.c_pix;
        d.y_base[(long long)y * d.y_row + (long long)x * d.y_pix] = col[0];
        d.u_base[c] = col[1];
        d.v_base[c] = col[2];
    } else {
        unsigned char* p = d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) p[d.ch_off[k]] = col[k];
    }
}

template <bool YUV>
__global__ __launch_bounds__(FD_THREADS) void face_draw_vertices_kernel(const typename DrDesc<YUV>::type* __restrict__ table, int q,
                                                                        FdFaces f, FdStyle st)
{
    const int s = blockIdx.y, j = blockIdx.x * FD_THREADS + threadIdx.x;
    if (f.slots[s] < 0) return;
    const typename DrDesc<YUV>::type& d = table[s / q];
    int cx, cy;
    if (!fd_vertex(f.pos + (size_t)s * FD_CELLS * 3, f.face_ind, f.V, st, j, &cx, &cy)) return;
    const int R = st.vertex_radius, H = d.H, W = d.W;
    const long long k = (long long)R * R + R;
    for (int y = cy - R; y <= cy + R; ++y)
        for (int x = cx - R; x <= cx + R; ++x)
            if (x >= 0 && x < W && y >= 0 && y < H && da_disc(x - cx, y - cy, k)) fd_store<YUV>(d, x, y, st.colors[2]);
}

template <bool YUV>
__global__ __launch_bounds__(FD_THREADS) void face_draw_kernel(const typename DrDesc<YUV>::type* __restrict__ table, int q,
                                                               const FdHeader* __restrict__ hdr, const DaPrim* __restrict__ prims, FdStyle st)
{
    constexpr int S = YUV ? 2 : 1, Q = S * S;
    const int n = blockIdx.z;
    const typename DrDesc<YUV>::type& d = table[n];
    const int H = d.H, W = d.W;
    const int tx0 = blockIdx.x * (FD_TILE * S), ty0 = blockIdx.y * (FD_TILE * S);
    if (tx0 >= W || ty0 >= H) return;                          // uniform over the block
    const int tx1 = min(tx0 + FD_TILE * S, W) - 1, ty1 = min(ty0 + FD_TILE * S, H) - 1;
    const int px = tx0 + (threadIdx.x % FD_TILE) * S, py = ty0 + (threadIdx.x / FD_TILE) * S;
    int win[Q];                                                // paint index (face * FD_STRIDE + primitive) of the pixel's winner, -1: none
#pragma unroll
    for (int k = 0; k < Q; ++k) win[k] = -1;
    for (int face = q - 1; face >= 0; --face) {
        const FdHeader h = hdr[(size_t)n * q + face];
        if (h.x0 > tx1 || h.x1 < tx0 || h.y0 > ty1 || h.y1 < ty0) continue;      // (an empty header rejects itself) uniform over the block
        const DaPrim* fp = prims + ((size_t)n * q + face) * FD_STRIDE;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const int x = px + (k % S), y = py + (k / S);
            if (win[k] >= 0 || x >= W || y >= H) continue;
            const int i = fd_face_winner(fp, h, st, x, y);
            if (i >= 0) win[k] = face * FD_STRIDE + i;
        }
    }
    if constexpr (YUV) {
        int top = -1;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            if (win[k] < 0) continue;
            const int x = px + (k % S), y = py + (k / S);
            d.y_base[(long long)y * d.y_row + (long long)x * d.y_pix] = st.colors[fd_class(win[k] % FD_STRIDE)][0];
            top = max(top, win[k]);
        }
        if (top >= 0) {
            const long long c = (long long)(py >> 1) * d.c_row + (long long)(px >> 1) * d.c_pix;
            const unsigned char* col = st.colors[fd_class(top % FD_STRIDE)];
            d.u_base[c] = col[1];
            d.v_base[c] = col[2];
        }
    } else {
        if (win[0] >= 0) fd_store<false>(d, px, py, st.colors[fd_class(win[0] % FD_STRIDE)]);
    }
}

#define FD_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" int cp_sizeof_face_style(void) { return (int)sizeof(FdStyle); }
extern "C" size_t cp_face_draw_scratch_bytes(int cap) { return fd_scratch_bytes(cap); }

extern "C" int cp_face_draw_frames_host(const void* table_host, int N, const int* slots, int cap, const float* landmarks, const int* box,
                                        const int* valid, const float* pos, const int* face_ind, int V, const void* style)
{
    const FdFaces f = {slots, landmarks, box, valid, pos, face_ind, V};
    FD_FORWARD(fd_draw_frames_host((const DrFrameDesc*)table_host, N, cap, f, (const FdStyle*)style, err, errn));
    return 0;
}

extern "C" int cp_face_draw_yuv_frames_host(const void* table_host, int N, const int* slots, int cap, const float* landmarks, const int* box,
                                            const int* valid, const float* pos, const int* face_ind, int V, const void* style)
{
    const FdFaces f = {slots, landmarks, box, valid, pos, face_ind, V};
    FD_FORWARD(fd_draw_yuv_frames_host((const DrYuvFrameDesc*)table_host, N, cap, f, (const FdStyle*)style, err, errn));
    return 0;
}

template <bool YUV>
static int fd_launch(const char* who, const void* table, const void* table_host, int N, int cap, const FdFaces& f, const FdStyle* st,
                     void* scratch, size_t scratch_bytes, void* stream)
{
    typedef typename DrDesc<YUV>::type Desc;
    FD_FORWARD(fd_check_call(who, N, cap, f, st, err, errn));
    CP_CHECK_ARG(table && table_host && scratch, "%s: null pointer", who);
    CP_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    CP_CHECK_ARG(scratch_bytes >= fd_scratch_bytes(cap), "%s: scratch of %zu bytes, %zu needed (cp_face_draw_scratch_bytes)", who, scratch_bytes,
                 fd_scratch_bytes(cap));
    const Desc* th = (const Desc*)table_host;
    if constexpr (YUV) {
        FD_FORWARD(dr_check_yuv_frames(who, th, N, err, errn));
    } else {
        FD_FORWARD(dr_check_frames(who, th, N, err, errn));
    }
    int maxH = 0, maxW = 0;
    for (int n = 0; n < N; ++n) {
        if (th[n].H > maxH) maxH = th[n].H;
        if (th[n].W > maxW) maxW = th[n].W;
    }
    hipStream_t s = (hipStream_t)stream;
    const int q = cap / N;
    FdHeader* hdr = (FdHeader*)scratch;
    DaPrim* prims = (DaPrim*)(hdr + cap);
    if (st->vertices) {
        const int count = fd_vertex_count(f.V, st->vertex_step);
        hipLaunchKernelGGL((face_draw_vertices_kernel<YUV>), dim3((unsigned)cp_cdiv(count, FD_THREADS), (unsigned)(N * q)), dim3(FD_THREADS), 0, s,
                           (const Desc*)table, q, f, *st);
        CP_CHECK_LAUNCH("face_draw_vertices_kernel");
    }
    hipLaunchKernelGGL(face_draw_build_kernel, dim3((unsigned)cap), dim3(FD_THREADS), 0, s, f, *st, hdr, prims);
    CP_CHECK_LAUNCH("face_draw_build_kernel");
    const int tile = FD_TILE * (YUV ? 2 : 1);
    const dim3 grid((unsigned)cp_cdiv(maxW, tile), (unsigned)cp_cdiv(maxH, tile), (unsigned)N);
    hipLaunchKernelGGL((face_draw_kernel<YUV>), grid, dim3(FD_THREADS), 0, s, (const Desc*)table, q, (const FdHeader*)hdr, (const DaPrim*)prims,
                       *st);
    CP_CHECK_LAUNCH("face_draw_kernel");
    cp_note_kernel(YUV ? "face_draw_kernel<yuv>" : "face_draw_kernel<bgr>");
    return 0;
}

extern "C" int cp_face_draw_frames_u8(const void* table, const void* table_host, int N, const int* slots, int cap, const float* landmarks,
                                      const int* box, const int* valid, const float* pos, const int* face_ind, int V, const void* style,
                                      void* scratch, size_t scratch_bytes, void* stream)
{
    const FdFaces f = {slots, landmarks, box, valid, pos, face_ind, V};
    return fd_launch<false>("face_draw_frames", table, table_host, N, cap, f, (const FdStyle*)style, scratch, scratch_bytes, stream);
}

extern "C" int cp_face_draw_yuv_frames_u8(const void* table, const void* table_host, int N, const int* slots, int cap, const float* landmarks,
                                          const int* box, const int* valid, const float* pos, const int* face_ind, int V, const void* style,
                                          void* scratch, size_t scratch_bytes, void* stream)
{
    const FdFaces f = {slots, landmarks, box, valid, pos, face_ind, V};
    return fd_launch<true>("face_draw_yuv_frames", table, table_host, N, cap, f, (const FdStyle*)style, scratch, scratch_bytes, stream);
}
