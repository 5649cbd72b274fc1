// draw_overlay: draw_results with a score label on every box and with translucent primitives -- the detections of N frames painted
// onto those frames, in place, on the device, as the reference's show_results does it: '{prefix}{score:.1f}' on a filled bar above the
// box (Debugger.add_coco_bbox) and the skeleton blended into the picture (Debugger.add_coco_hp).  The picture is defined by
// draw_overlay_arith.h: the coverage tests and painter's order of draw_arith.h, two more primitives per row for the label, and an
// integer blend per covering primitive.  The rows stay on the device: the score becomes glyphs inside the build kernel.
//
//   cp_draw_overlay_frames_u8      : frames addressed by cp_frame_desc (packed / planar BGR or RGB, 3 or 4 channels, any positive strides)
//   cp_draw_overlay_yuv_frames_u8  : frames addressed by cp_yuv_frame_desc (NV12 / NV21 / I420 planes), colours given as (Y, U, V)
//   cp_draw_overlay_frames_host / cp_draw_overlay_yuv_frames_host : the sequential HOST painters of draw_overlay_host.h, same statements
//   cp_draw_score_label            : the score rule, one value at a time
//
// Two launches per call, as for draw_results:
//   1. draw_overlay_build_kernel  one wave per row; lane l < 36 builds primitive l, lane 36 the label record (the glyphs of prefix and
//                                 score, the bar's corner); a ballot gives the mask of the primitives that exist (38 bits) and a wave
//                                 reduction the row's bounding box, the bar included.
//   2. draw_overlay_kernel        the tile and ownership of draw_raster_kernel: one pixel per thread for BGR, one 2x2 block with its
//                                 chroma sample for YUV, so every read-modify-write stays inside one thread.  A block walks the rows
//                                 from the back and finds per owned pixel the topmost OPAQUE cover (opacity 256: what draw_raster_kernel
//                                 finds); if the style has a translucent class it walks them once more forward and blends, per pixel,
//                                 the translucent primitives that lie above that cover.  A pixel is read only where a translucent
//                                 primitive covers it and nothing opaque lies beneath; what only opaque paint covers is stored as before.
// Byte loads and stores from plain C++ only.  Compiled with -ffp-contract=off like the other pre / post stages.
#include "common.h"
#include "draw_overlay_host.h"

#define DV_THREADS 256
#define DV_TILE 16      // a block is DV_TILE x DV_TILE threads; a thread owns one pixel (BGR) or one 2x2 block (YUV)

__global__ __launch_bounds__(DV_THREADS) void draw_overlay_build_kernel(const float* __restrict__ rows, long long total, float vis_thresh,
                                                                        int box_thickness, int limb_radius, int joint_radius, DoOverlay ov,
                                                                        DrRowHeader* __restrict__ hdr, DaPrim* __restrict__ prims,
                                                                        DoLabel* __restrict__ labels)
{
    const long long r = (long long)blockIdx.x * (DV_THREADS / CP_WAVE) + (threadIdx.x / CP_WAVE);
    if (r >= total) return;                                    // uniform over the wave
    const int lane = threadIdx.x % CP_WAVE;
    const float* row = rows + r * DA_ROW;
    const bool live = da_live(row, vis_thresh);
    DaPrim p = {0, 0, 0, 0};
    bool ok = false;
    int reach = 0;
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    if (lane < DA_PRIMS && live) {
        reach = da_reach(box_thickness, limb_radius, joint_radius, lane);
        ok = reach >= 0 && da_build(row, lane, &p);
        if (ok) {
            da_bounds(p, reach, &x0, &y0, &x1, &y1);
            prims[r * DA_PRIMS + lane] = p;
        }
    }
    if (lane == DO_BAR) {
        DoLabel lb;
        ok = do_build_label(row, ov, &lb) && live;
        if (!ok) lb.nchars = 0;
        else do_label_bounds(lb, ov.label_scale, &x0, &y0, &x1, &y1);
        labels[r] = lb;
    }
    unsigned long long mask = __ballot(ok);
    mask |= ((mask >> DO_BAR) & 1) << DO_TEXT;
#pragma unroll
    for (int s = CP_WAVE / 2; s > 0; s >>= 1) {
        x0 = min(x0, __shfl_xor(x0, s)); y0 = min(y0, __shfl_xor(y0, s));
        x1 = max(x1, __shfl_xor(x1, s)); y1 = max(y1, __shfl_xor(y1, s));
    }
    if (lane == 0) hdr[r] = DrRowHeader{x0, y0, x1, y1, mask, 0};
}

template <bool YUV>
__global__ __launch_bounds__(DV_THREADS) void draw_overlay_kernel(const typename DrDesc<YUV>::type* __restrict__ table,
                                                                  const DrRowHeader* __restrict__ hdr, const DaPrim* __restrict__ prims,
                                                                  const DoLabel* __restrict__ labels, int M, DaStyle st, DoOverlay ov,
                                                                  const int* __restrict__ row_ids, DaIdPalette idp)
{
    constexpr int S = YUV ? 2 : 1, Q = S * S, C = YUV ? 1 : 3;
    const typename DrDesc<YUV>::type& d = table[blockIdx.z];
    const int H = d.H, W = d.W;
    const int tx0 = blockIdx.x * (DV_TILE * S), ty0 = blockIdx.y * (DV_TILE * S);
    if (tx0 >= W || ty0 >= H) return;                          // uniform over the block
    const int tx1 = min(tx0 + DV_TILE * S, W) - 1, ty1 = min(ty0 + DV_TILE * S, H) - 1;
    const int tid = threadIdx.x, lane = tid % CP_WAVE, wave = tid / CP_WAVE;
    const int px = tx0 + (tid % DV_TILE) * S, py = ty0 + (tid / DV_TILE) * S;
    const int T = st.box_thickness, RL = st.limb_radius, RJ = st.joint_radius, fs = ov.label_scale;
    const DrRowHeader* fh = hdr + (size_t)blockIdx.z * M;
    const DaPrim* fp = prims + (size_t)blockIdx.z * M * DA_PRIMS;
    const DoLabel* fl = labels + (size_t)blockIdx.z * M;
    const unsigned long long opaque = do_opaque_mask(ov);

    __shared__ int list[DV_THREADS];
    __shared__ int wcount[DV_THREADS / CP_WAVE];

    // the rows base .. base + 255 whose bounding box meets the tile, compacted into `list` in order -> how many (uniform over the block)
    auto compact = [&](int base) -> int {
        const int m = base + tid;
        bool hit = false;
        if (m < M) {
            const DrRowHeader h = fh[m];
            hit = h.x0 <= tx1 && h.x1 >= tx0 && h.y0 <= ty1 && h.y1 >= ty0;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(b);
        __syncthreads();
        int before = 0, count = 0;
#pragma unroll
        for (int w = 0; w < DV_THREADS / CP_WAVE; ++w) {
            before += w < wave ? wcount[w] : 0;
            count += wcount[w];
        }
        if (hit) list[before + __popcll(b & ((1ull << lane) - 1))] = m;
        __syncthreads();
        return count;
    };

    bool inside[Q];                                            // whether the thread's pixel q lies in the frame
    int win[Q];                                                // paint index (row * 38 + primitive) of the pixel's topmost opaque cover, -1: none
    int open = 0;                                              // pixels of this thread that lie in the frame and have no such cover yet
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        win[q] = -1;
        inside[q] = px + (q % S) < W && py + (q / S) < H;
        open += inside[q] ? 1 : 0;
    }

    for (int base = ((M - 1) / DV_THREADS) * DV_THREADS; base >= 0; base -= DV_THREADS) {
        const int count = compact(base);
        for (int i = count - 1; i >= 0 && open > 0; --i) {
            const int r = list[i];
            const unsigned long long mask = fh[r].mask & opaque;
            if (!mask) continue;
            const DaPrim* rp = fp + (size_t)r * DA_PRIMS;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (win[q] >= 0 || !inside[q]) continue;
                const int l = do_row_winner(rp, fl[r], mask, T, RL, RJ, fs, px + (q % S), py + (q / S));
                if (l >= 0) {
                    win[q] = r * DO_PRIMS + l;
                    --open;
                }
            }
        }
        __syncthreads();                                       // the list is rewritten by the next chunk
    }

    // what the primitive with paint index w stores
    auto color = [&](int w, int* c) {
        const int id = row_ids ? row_ids[(size_t)blockIdx.z * M + w / DO_PRIMS] : -1;
        do_color(st, ov, row_ids ? &idp : nullptr, id, w % DO_PRIMS, c);
    };
    // where channel k of pixel q lives (YUV: its luma byte)
    auto at = [&](int q, int k) -> unsigned char* {
        const int x = px + (q % S), y = py + (q / S);
        if constexpr (YUV)
            return d.y_base + (long long)y * d.y_row + (long long)x * d.y_pix;
        else
            return d.base + (long long)y * d.row_stride + (long long)x * d.pix_stride + d.ch_off[k];
    };

    int val[Q][C];                                             // the bytes of pixel q as painted so far ...
    bool have[Q];                                              // ... once something was painted on it
    int cu = 0, cv = 0, top = -1;                              // YUV: the chroma sample, and the topmost opaque cover of its block
    bool chave = false;
    int low = INT32_MAX;                                       // the lowest of the covers: nothing at or below it is blended by this thread
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        have[q] = win[q] >= 0;
#pragma unroll
        for (int k = 0; k < C; ++k) val[q][k] = 0;
        if (have[q]) {
            int col[3];
            color(win[q], col);
#pragma unroll
            for (int k = 0; k < C; ++k) val[q][k] = col[k];
        }
        top = max(top, win[q]);
        if (inside[q]) low = min(low, win[q]);
    }
    if constexpr (YUV) {
        if (top >= 0) {
            int col[3];
            color(top, col);
            cu = col[1];
            cv = col[2];
            chave = true;
        }
    }

    if (opaque != (1ull << DO_PRIMS) - 1) {                    // a translucent class: uniform over the grid
        for (int base = 0; base < M; base += DV_THREADS) {
            const int count = compact(base);
            for (int i = 0; i < count; ++i) {
                const int r = list[i];
                unsigned long long tm = fh[r].mask & ~opaque;
                if (!tm || r * DO_PRIMS + (DO_PRIMS - 1) <= low) continue;
                const DaPrim* rp = fp + (size_t)r * DA_PRIMS;
                while (tm) {
                    const int l = __ffsll(tm) - 1;             // < 36: the label is opaque
                    tm &= tm - 1;
                    const int w = r * DO_PRIMS + l, a = do_opacity(ov, l);
                    const DaPrim p = rp[l];
                    int col[3] = {0, 0, 0};
                    bool any = false;
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        if (!inside[q] || w <= win[q] || !da_covers(p, l, T, RL, RJ, px + (q % S), py + (q / S))) continue;
                        if (!any) color(w, col);
                        if (!have[q]) {
#pragma unroll
                            for (int k = 0; k < C; ++k) val[q][k] = *at(q, k);
                            have[q] = true;
                        }
#pragma unroll
                        for (int k = 0; k < C; ++k) val[q][k] = do_blend(val[q][k], col[k], a);
                        any = true;
                    }
                    if constexpr (YUV) {
                        if (any && w > top) {                  // w > top: every in-frame pixel of the block was tested
                            if (!chave) {
                                const long long c = (long long)(py >> 1) * d.c_row + (long long)(px >> 1) * d.c_pix;
                                cu = d.u_base[c];
                                cv = d.v_base[c];
                                chave = true;
                            }
                            cu = do_blend(cu, col[1], a);
                            cv = do_blend(cv, col[2], a);
                        }
                    }
                }
            }
            __syncthreads();                                   // the list is rewritten by the next chunk
        }
    }

#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (!have[q]) continue;
#pragma unroll
        for (int k = 0; k < C; ++k) *at(q, k) = (unsigned char)val[q][k];
    }
    if constexpr (YUV) {
        if (chave) {
            const long long c = (long long)(py >> 1) * d.c_row + (long long)(px >> 1) * d.c_pix;
            d.u_base[c] = (unsigned char)cu;
            d.v_base[c] = (unsigned char)cv;
        }
    }
}

extern "C" int cp_sizeof_draw_overlay(void) { return (int)sizeof(DoOverlay); }
extern "C" size_t cp_draw_overlay_scratch_bytes(int N, int M) { return do_scratch_bytes(N, M); }

extern "C" int cp_draw_score_label(float score, unsigned char* glyphs)
{
    unsigned char g[6];
    const int n = do_score_glyphs(score, g);
    for (int i = 0; i < n && glyphs; ++i) glyphs[i] = g[i];
    return n;
}

#define DV_FORWARD(call)                          \
    do {                                          \
        char err[256];                            \
        const size_t errn = sizeof(err);          \
        err[0] = 0;                               \
        if (int rc = (call)) {                    \
            cp_set_error("%s", err);              \
            return rc;                            \
        }                                         \
    } while (0)

extern "C" int cp_draw_overlay_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                           const int* row_ids, const void* id_palette, const void* overlay)
{
    DV_FORWARD(do_draw_frames_host<false>((const DrFrameDesc*)table_host, N, rows, M, vis_thresh, (const DaStyle*)style, row_ids,
                                          (const DaIdPalette*)id_palette, (const DoOverlay*)overlay, err, errn));
    return 0;
}

extern "C" int cp_draw_overlay_yuv_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                               const int* row_ids, const void* id_palette, const void* overlay)
{
    DV_FORWARD(do_draw_frames_host<true>((const DrYuvFrameDesc*)table_host, N, rows, M, vis_thresh, (const DaStyle*)style, row_ids,
                                         (const DaIdPalette*)id_palette, (const DoOverlay*)overlay, err, errn));
    return 0;
}

template <bool YUV>
static int dv_launch(const char* who, const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                     const DaStyle* style, void* scratch, size_t scratch_bytes, const int* row_ids, const DaIdPalette* idp, const DoOverlay* ov,
                     void* stream)
{
    typedef typename DrDesc<YUV>::type Desc;
    bool noop;
    DV_FORWARD(dr_check_call(who, N, M, vis_thresh, style, &noop, err, errn));
    DV_FORWARD(do_check_overlay(who, ov, err, errn));
    if (noop) return 0;
    DV_FORWARD(do_check_ids(who, row_ids, idp, err, errn));
    CP_CHECK_ARG(table && table_host && rows && scratch, "%s: null pointer", who);
    CP_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    CP_CHECK_ARG(scratch_bytes >= do_scratch_bytes(N, M), "%s: scratch of %zu bytes, %zu needed (cp_draw_overlay_scratch_bytes)", who,
                 scratch_bytes, do_scratch_bytes(N, M));
    const Desc* th = (const Desc*)table_host;
    if constexpr (YUV) {
        DV_FORWARD(dr_check_yuv_frames(who, th, N, err, errn));
    } else {
        DV_FORWARD(dr_check_frames(who, th, N, err, errn));
    }
    int maxH = 0, maxW = 0;
    for (int n = 0; n < N; ++n) {
        if (th[n].H > maxH) maxH = th[n].H;
        if (th[n].W > maxW) maxW = th[n].W;
    }
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)N * M;
    DrRowHeader* hdr = (DrRowHeader*)scratch;
    DaPrim* prims = (DaPrim*)(hdr + total);
    DoLabel* labels = (DoLabel*)(prims + total * DA_PRIMS);
    const int per_block = DV_THREADS / CP_WAVE;
    hipLaunchKernelGGL(draw_overlay_build_kernel, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(DV_THREADS), 0, s, rows, total,
                       vis_thresh, style->box_thickness, style->limb_radius, style->joint_radius, *ov, hdr, prims, labels);
    CP_CHECK_LAUNCH("draw_overlay_build_kernel");
    const int tile = DV_TILE * (YUV ? 2 : 1);
    const dim3 grid((unsigned)cp_cdiv(maxW, tile), (unsigned)cp_cdiv(maxH, tile), (unsigned)N);
    DaIdPalette none = {};
    hipLaunchKernelGGL((draw_overlay_kernel<YUV>), grid, dim3(DV_THREADS), 0, s, (const Desc*)table, (const DrRowHeader*)hdr,
                       (const DaPrim*)prims, (const DoLabel*)labels, M, *style, *ov, row_ids, idp ? *idp : none);
    CP_CHECK_LAUNCH("draw_overlay_kernel");
    cp_note_kernel(YUV ? "draw_overlay_kernel<yuv>" : "draw_overlay_kernel<bgr>");
    return 0;
}

// table DEVICE, table_host HOST; rows DEVICE float32 [N,M,56]; style, id_palette, overlay HOST; row_ids DEVICE int [N,M] or null with a
// null id_palette; scratch DEVICE, 16-byte aligned, at least cp_draw_overlay_scratch_bytes(N, M) bytes
extern "C" int cp_draw_overlay_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                         const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                                         const void* overlay, void* stream)
{
    return dv_launch<false>("draw_overlay_frames", table, table_host, N, rows, M, vis_thresh, (const DaStyle*)style, scratch, scratch_bytes,
                            row_ids, (const DaIdPalette*)id_palette, (const DoOverlay*)overlay, stream);
}

extern "C" int cp_draw_overlay_yuv_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                             const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                                             const void* overlay, void* stream)
{
    return dv_launch<true>("draw_overlay_yuv_frames", table, table_host, N, rows, M, vis_thresh, (const DaStyle*)style, scratch, scratch_bytes,
                           row_ids, (const DaIdPalette*)id_palette, (const DoOverlay*)overlay, stream);
}
