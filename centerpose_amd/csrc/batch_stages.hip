// The stages around the network for N images at once on gfx950 (MultiPoseDetector.run_batch).
//
//   cp_preprocess_batch_u8_f32 : cv2.resize + cv2.warpAffine + normalise + HWC->CHW (+ mirrored twin) of base_detector.py:47-58 for N
//                                source images of different sizes in one resize launch (when any image needs it) and one warp launch.
//   cp_post_merge_batch_f32    : the inverse affine of multi_pose.py:62-71 for S scales x N images, the concatenation of the scales
//                                (multi_pose.py:73-75) and soft_nms_39 (lib/external/nms.pyx:172-275) per image, in one launch.
//
// The arithmetic is that of prepost.hip (resize_u8_kernel, preprocess_kernel, transform_dets_kernel) and of host_nms.cpp, statement for
// statement (the pre-process statements live in pre_arith.h, shared with frame_sources.hip): batched results are bit-identical to the
// per-image calls.  The one exception is the Gaussian weight of soft-NMS method 2, (float)exp((double)x): the device's double exp is
// not guaranteed to round like the host C library's, so a decayed score (column 4) may differ in its last float bit per decay.  Compiled with -ffp-contract=off: the coordinate and box arithmetic must round like the host
// C++ it restates (host_nms.cpp is built for x86-64, which contracts nothing).
#include <cmath>
#include "common.h"
#include "pre_arith.h"

// ---------------------------------------------------------------------------------------------------- batched pre-process
// mirror of cp_pre_desc (include/centerpose_hip.h)
struct PreDesc {
    long long src_off;      // byte offset of the uint8 [H,W,3] image in the staging buffer
    long long mid_off;      // byte offset of the resized uint8 [NH,NW,3] image in the scratch buffer, < 0: (NH,NW) == (H,W), no resize
    int H, W, NH, NW;
    double mi[6];           // INVERTED warp matrix: destination pixel -> coordinates in the (resized) image
    int slot, pad;          // output batch index of the image (its mirrored twin goes to slot + 1)
};

// blockIdx.y: image; blockIdx.x: grid-stride tiles of its resized pixels.  Images without a resize leave at once.
__global__ __launch_bounds__(BS_THREADS) void resize_batch_u8_kernel(const unsigned char* __restrict__ staging, unsigned char* __restrict__ scratch,
                                                                     const PreDesc* __restrict__ table)
{
    const PreDesc& d = table[blockIdx.y];
    if (d.mid_off < 0) return;
    const int H = d.H, W = d.W, NH = d.NH, NW = d.NW, total = NH * NW;
    const double scale_x = (double)W / NW, scale_y = (double)H / NH;
    const BsPacked src = {staging + d.src_off, W};
    unsigned char* dst = scratch + d.mid_off;
    for (int i = blockIdx.x * BS_THREADS + threadIdx.x; i < total; i += gridDim.x * BS_THREADS) {
        const int dy = i / NW, dx = i - dy * NW;
        bs_resize_pixel(src, H, W, scale_x, scale_y, dx, dy, dst + (size_t)i * 3);
    }
}

// blockIdx.y: image; blockIdx.x: grid-stride tiles of its OH x OW destination pixels (bs_warp_image, pre_arith.h).
template <bool VEC>
__global__ __launch_bounds__(BS_THREADS) void preprocess_batch_kernel(const unsigned char* __restrict__ staging,
                                                                      const unsigned char* __restrict__ scratch,
                                                                      const PreDesc* __restrict__ table, float* __restrict__ out, int OH, int OW,
                                                                      BsNorm nm, int flip)
{
    const PreDesc& d = table[blockIdx.y];
    const BsPacked src = {d.mid_off < 0 ? staging + d.src_off : scratch + d.mid_off, d.NW};
    double m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = d.mi[k];
    const size_t total = (size_t)OH * OW;
    float* o = out + (size_t)d.slot * 3 * total;
    bs_warp_image<VEC>(src, d.NH, d.NW, m, o, o + 3 * total, OH, OW, nm, flip);
}

extern "C" int cp_sizeof_pre_desc(void) { return (int)sizeof(PreDesc); }

// The inversion cv::warpAffine applies to its matrix argument, with the double operations of cp_preprocess_u8_f32 (prepost.hip).
extern "C" int cp_invert_warp(const double* M /* host 2x3 */, double* Mi /* host 2x3 */)
{
    CP_CHECK_ARG(M && Mi, "invert_warp: bad arguments");
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    Mi[0] = A11; Mi[1] = M[1] * -D;
    Mi[3] = M[3] * -D; Mi[4] = A22;
    Mi[2] = -Mi[0] * M[2] - Mi[1] * M[5];
    Mi[5] = -Mi[3] * M[2] - Mi[4] * M[5];
    return 0;
}

// table / table_host: the same N descriptors on the device and on the host (the host copy is what the bounds are checked against).
extern "C" int cp_preprocess_batch_u8_f32(const unsigned char* staging, size_t staging_bytes, unsigned char* scratch, size_t scratch_bytes,
                                          const void* table, const void* table_host, int N, float* out, int out_batch, int OH, int OW,
                                          const float* mean /* host 3 */, const float* std_ /* host 3 */, int flip, void* stream)
{
    CP_CHECK_ARG(staging && table && table_host && out && mean && std_ && N > 0 && OH > 0 && OW > 0 && out_batch > 0,
                 "preprocess_batch: bad arguments");
    CP_CHECK_ARG(N <= 65535, "preprocess_batch: at most 65535 images per launch (got %d)", N);
    CP_CHECK_ARG((long long)OH * OW < (1ll << 29), "preprocess_batch: output %d x %d too large", OH, OW);
    const PreDesc* th = (const PreDesc*)table_host;
    const int nb = flip ? 2 : 1;
    long long max_resized = 0;
    for (int n = 0; n < N; ++n) {
        const PreDesc& d = th[n];
        CP_CHECK_ARG(d.H > 0 && d.W > 0 && d.NH > 0 && d.NW > 0 && (long long)d.H * d.W < (1ll << 29) && (long long)d.NH * d.NW < (1ll << 29),
                     "preprocess_batch: image %d: bad size %d x %d -> %d x %d", n, d.H, d.W, d.NH, d.NW);
        const long long src_bytes = (long long)d.H * d.W * 3, mid_bytes = (long long)d.NH * d.NW * 3;
        CP_CHECK_ARG(d.src_off >= 0 && d.src_off + src_bytes <= (long long)staging_bytes, "preprocess_batch: image %d lies outside the staging buffer", n);
        if (d.mid_off >= 0) {
            CP_CHECK_ARG(scratch && d.mid_off + mid_bytes <= (long long)scratch_bytes, "preprocess_batch: image %d: resized image lies outside the scratch buffer", n);
            if ((long long)d.NH * d.NW > max_resized) max_resized = (long long)d.NH * d.NW;
        } else {
            CP_CHECK_ARG(d.NH == d.H && d.NW == d.W, "preprocess_batch: image %d: %d x %d -> %d x %d needs a scratch offset", n, d.H, d.W, d.NH, d.NW);
        }
        CP_CHECK_ARG(d.slot >= 0 && d.slot + nb <= out_batch, "preprocess_batch: image %d: output slot %d outside the batch of %d", n, d.slot, out_batch);
    }
    hipStream_t s = (hipStream_t)stream;
    if (max_resized > 0) {
        long long gx = (max_resized + BS_THREADS - 1) / BS_THREADS;
        if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(resize_batch_u8_kernel, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, staging, scratch, (const PreDesc*)table);
        CP_CHECK_LAUNCH("resize_batch_u8_kernel");
    }
    BsNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.sd[c] = std_[c]; }
    const bool vec = OW % 4 == 0 && ((size_t)out & 15) == 0;
    long long gx = ((long long)OH * (vec ? OW / 4 : OW) + BS_THREADS - 1) / BS_THREADS;
    if (gx > 4096) gx = 4096;
    if (vec)
        hipLaunchKernelGGL(preprocess_batch_kernel<true>, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, staging, scratch,
                           (const PreDesc*)table, out, OH, OW, nm, flip ? 1 : 0);
    else
        hipLaunchKernelGGL(preprocess_batch_kernel<false>, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, staging, scratch,
                           (const PreDesc*)table, out, OH, OW, nm, flip ? 1 : 0);
    CP_CHECK_LAUNCH("preprocess_batch_kernel");
    cp_note_kernel(vec ? "preprocess_batch_kernel<vec4>" : "preprocess_batch_kernel<scalar>");
    return 0;
}

// ---------------------------------------------------------------------------------------------------- batched post-process + soft-NMS
#define PM_MAX_SCALES 4
#define PM_MAX_ROWS 512
#define PM_D 56             // 5 + 3 * 17
#define PM_MOVE 39          // soft_nms_39: columns 0..38 move with a row
#define PM_STRIDE 57        // LDS row stride in floats: odd, so a column read over consecutive rows is free of bank conflicts
#define PM_LANES 64         // one wave per image: the discard compaction is sequential, a barrier costs nothing in a one-wave workgroup

struct PostMergeArgs {
    const float* dets[PM_MAX_SCALES];      // [N,K,56] per scale
    float scale[PM_MAX_SCALES];
    const double* trans;                   // device [S][N][6] feature-map -> image, or NULL: rows are taken as they are
    float* out;                            // [N, S*K, 56], scale-major per image
    int* n_keep;                           // [N]
    int S, N, K, method;
    float sigma, Nt, threshold;
};

// element c of merged row r of image n: transform_dets_kernel's arithmetic (prepost.hip)
__device__ __forceinline__ float pm_value(const PostMergeArgs& a, int n, int r, int c)
{
    const int s = r / a.K, k = r - s * a.K;
    const float* base = a.dets[0];
    float scale = a.scale[0];
#pragma unroll
    for (int q = 1; q < PM_MAX_SCALES; ++q)
        if (q == s) { base = a.dets[q]; scale = a.scale[q]; }
    const float* row = base + ((size_t)n * a.K + k) * PM_D;
    float v = row[c];
    if (a.trans && (c < 4 || (c >= 5 && c < PM_MOVE))) {
        const int cc = c < 4 ? c : c - 5;
        const int xi = (c < 4 ? 0 : 5) + (cc & ~1);
        const double x = (double)row[xi], y = (double)row[xi + 1];
        const double* t = a.trans + ((size_t)s * a.N + n) * 6 + ((cc & 1) ? 3 : 0);
        v = (float)(t[0] * x + t[1] * y + t[2]) / scale;
    }
    return v;
}

// no NMS: the transformed rows of every scale, concatenated per image
__global__ __launch_bounds__(BS_THREADS) void post_concat_kernel(const PostMergeArgs a)
{
    const int R = a.S * a.K, per = R * PM_D, total = a.N * per;
    for (int i = blockIdx.x * BS_THREADS + threadIdx.x; i < total; i += gridDim.x * BS_THREADS) {
        const int n = i / per, e = i - n * per, r = e / PM_D;
        a.out[i] = pm_value(a, n, r, e - r * PM_D);
        if (e == 0) a.n_keep[n] = R;
    }
}

// soft_nms_39 of host_nms.cpp, one wave per image, the image's R rows in LDS.  Per outer step i: the arg-max over rows i..N-1 (strict <:
// the lowest index wins a tie) and the decayed score of every row behind i are parallel over the rows; the decayed scores are parked
// beside the rows (ns / fl) and committed in the order the host loop visits them, because a discard moves the LAST row -- not visited
// yet, its score still undecayed -- into the discarded slot, where it is examined next, and leaves the last slot's columns 0..4 as
// they were.  Between two discards the commits are independent and run in parallel.
__global__ __launch_bounds__(PM_LANES) void post_merge_nms_kernel(const PostMergeArgs a)
{
    extern __shared__ float pm_lds[];
    const int R = a.S * a.K, n = blockIdx.x, lane = threadIdx.x;
    float* rows = pm_lds;                              // [R][PM_STRIDE]
    float* ns = pm_lds + (size_t)R * PM_STRIDE;        // [R] decayed score of a row that overlaps the current box
    int* fl = (int*)(ns + R);                          // [R] bit 0: overlaps (ns valid), bit 1: falls under the threshold
    for (int e = lane; e < R * PM_D; e += PM_LANES) {
        const int r = e / PM_D, c = e - r * PM_D;
        rows[r * PM_STRIDE + c] = pm_value(a, n, r, c);
    }
    __syncthreads();
    int N = R;
    for (int i = 0; i + 1 < N; ++i) {                  // i >= N - 1 changes nothing on the host either, and N only shrinks
        // arg-max: host scan `if (maxscore < s[pos])` from maxscore = s[i] == the lowest index of the maximum, unless s[i] is not below it
        const float si = rows[i * PM_STRIDE + 4];
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int pos = i + 1 + lane; pos < N; pos += PM_LANES) {
            const float s = rows[pos * PM_STRIDE + 4];
            if (s > bv) { bv = s; bi = pos; }
        }
#pragma unroll
        for (int off = 1; off < PM_LANES; off <<= 1) {
            const float ov = __shfl_xor(bv, off, PM_LANES);
            const int oi = __shfl_xor(bi, off, PM_LANES);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        const int maxpos = si < bv ? bi : i;
        if (maxpos != i && lane < PM_MOVE) {
            const float t = rows[i * PM_STRIDE + lane];
            rows[i * PM_STRIDE + lane] = rows[maxpos * PM_STRIDE + lane];
            rows[maxpos * PM_STRIDE + lane] = t;
        }
        __syncthreads();
        const float tx1 = rows[i * PM_STRIDE], ty1 = rows[i * PM_STRIDE + 1], tx2 = rows[i * PM_STRIDE + 2], ty2 = rows[i * PM_STRIDE + 3];
        for (int pos = i + 1 + lane; pos < N; pos += PM_LANES) {
            const float* r = rows + pos * PM_STRIDE;
            const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
            const float area = (x2 - x1 + 1) * (y2 - y1 + 1);
            const float iw = fminf(tx2, x2) - fmaxf(tx1, x1) + 1;
            int f = 0;
            float v = 0.f;
            if (iw > 0) {
                const float ih = fminf(ty2, y2) - fmaxf(ty1, y1) + 1;
                if (ih > 0) {
                    const float ua = (tx2 - tx1 + 1) * (ty2 - ty1 + 1) + area - iw * ih;
                    const float ov = iw * ih / ua;
                    float weight;
                    if (a.method == 1) weight = ov > a.Nt ? 1 - ov : 1;
                    else if (a.method == 2) weight = (float)exp((double)(-(ov * ov) / a.sigma));
                    else weight = ov > a.Nt ? 0 : 1;
                    v = weight * r[4];
                    f = v < a.threshold ? 3 : 1;
                }
            }
            ns[pos] = v;
            fl[pos] = f;
        }
        __syncthreads();
        int pos = i + 1;
        for (;;) {
            int p = 0x7fffffff;                        // the next row at or behind pos that is discarded
            for (int q = pos + lane; q < N; q += PM_LANES)
                if (fl[q] & 2) { p = q; break; }
#pragma unroll
            for (int off = 1; off < PM_LANES; off <<= 1) p = min(p, __shfl_xor(p, off, PM_LANES));
            const int end = p < N ? p : N;
            for (int q = pos + lane; q < end; q += PM_LANES)
                if (fl[q]) rows[q * PM_STRIDE + 4] = ns[q];
            if (p >= N) break;
            // row p: r[4] = decayed, then columns 0..4 <- last row's (a copy), columns 5..38 swapped with it; the row that came in
            // carries its parked score and is examined at p
            const int last = N - 1;
            if (lane < 4) rows[p * PM_STRIDE + lane] = rows[last * PM_STRIDE + lane];
            else if (lane == 4) rows[p * PM_STRIDE + 4] = p == last ? ns[p] : rows[last * PM_STRIDE + 4];
            else if (lane < PM_MOVE) {
                const float t = rows[p * PM_STRIDE + lane];
                rows[p * PM_STRIDE + lane] = rows[last * PM_STRIDE + lane];
                rows[last * PM_STRIDE + lane] = t;
            } else if (lane == PM_MOVE) {
                ns[p] = ns[last];
                fl[p] = fl[last];
            }
            --N;
            pos = p;
            __syncthreads();
        }
        __syncthreads();
    }
    __syncthreads();
    float* o = a.out + (size_t)n * R * PM_D;
    for (int e = lane; e < R * PM_D; e += PM_LANES) {
        const int r = e / PM_D, c = e - r * PM_D;
        o[e] = rows[r * PM_STRIDE + c];
    }
    if (lane == 0) a.n_keep[n] = N;
}

extern "C" int cp_post_merge_max_rows(void) { return PM_MAX_ROWS; }

// dets: S host pointers to DEVICE float32 [N,K,56]; trans: DEVICE double [S][N][6] (feature map -> image) or NULL when the rows are
// mapped already; scales: HOST float[S] (read with trans); out: DEVICE [N,S*K,56]; n_keep: DEVICE int[N].
extern "C" int cp_post_merge_batch_f32(int S, const float* const* dets, const double* trans, const float* scales, int N, int K, float* out,
                                       int* n_keep, int nms, float sigma, float Nt, float threshold, int method, void* stream)
{
    CP_CHECK_ARG(S >= 1 && S <= PM_MAX_SCALES, "post_merge_batch: 1..%d scales (got %d)", PM_MAX_SCALES, S);
    CP_CHECK_ARG(dets && out && n_keep && N >= 1 && K >= 1, "post_merge_batch: bad arguments");
    CP_CHECK_ARG(!trans || scales, "post_merge_batch: the affine needs the scales");
    CP_CHECK_ARG((long long)N * S * K * PM_D < (1ll << 31), "post_merge_batch: too many rows");
    PostMergeArgs a;
    for (int s = 0; s < PM_MAX_SCALES; ++s) {
        const int ss = s < S ? s : 0;
        CP_CHECK_ARG(dets[ss], "post_merge_batch: scale %d: no detections", ss);
        a.dets[s] = dets[ss];
        a.scale[s] = trans ? scales[ss] : 1.f;
        CP_CHECK_ARG(a.scale[s] > 0.f, "post_merge_batch: scale %d: bad scale", ss);
    }
    a.trans = trans; a.out = out; a.n_keep = n_keep;
    a.S = S; a.N = N; a.K = K; a.method = method;
    a.sigma = sigma; a.Nt = Nt; a.threshold = threshold;
    hipStream_t st = (hipStream_t)stream;
    if (!nms) {
        const int total = N * S * K * PM_D;
        int grid = (total + BS_THREADS - 1) / BS_THREADS;
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(post_concat_kernel, dim3(grid), dim3(BS_THREADS), 0, st, a);
        CP_CHECK_LAUNCH("post_concat_kernel");
        return 0;
    }
    const int R = S * K;
    CP_CHECK_ARG(R <= PM_MAX_ROWS, "post_merge_batch: soft-NMS holds an image's rows in LDS: at most %d rows per image (got %d = %d scales x %d)",
                 PM_MAX_ROWS, R, S, K);
    CP_CHECK_ARG(method >= 0 && method <= 2, "post_merge_batch: soft-NMS method 0, 1 or 2 (got %d)", method);
    const int smem = R * (PM_STRIDE + 2) * 4;
    static CpLdsGuard guard;
    if (smem > 64 * 1024) {
        const hipError_t e = guard.ensure((const void*)post_merge_nms_kernel, smem);
        if (e != hipSuccess) { cp_set_error("post_merge_batch: cannot reserve %d B LDS: %s", smem, hipGetErrorString(e)); return 2; }
    }
    hipLaunchKernelGGL(post_merge_nms_kernel, dim3(N), dim3(PM_LANES), smem, st, a);
    CP_CHECK_LAUNCH("post_merge_nms_kernel");
    return 0;
}
