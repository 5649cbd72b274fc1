// Detections-only head evaluation on gfx950: the wh / hps / reg branches of the KeypointHead at the decoded person-centre
// peaks and the hp_offset branch at the decoded joint peaks -- the only pixels multi_pose_decode reads of those four maps
// (lib/models/decode.py:240-307; pose_assign_kernel in decode.hip).  Each branch is
//   3x3 conv (C -> hc) + bias + ReLU -> 1x1 conv (hc -> n) + bias      (lib/models/heads/keypoint.py:14-37)
// evaluated as a GATHERED implicit GEMM: M = points, N = hc hidden channels, K = 9 * C (tap-major, channel-minor, the order of
// the dense direct kernel's packed weights).
//
// One block = 32 points x one branch x all hc hidden channels, so the 1x1 runs on the block's own hidden tile:
//   * per tap, the 32 points' C-float NHWC rows are gathered into LDS (zeros outside the map: the dense conv's padding);
//   * every wave owns NS 32-wide hidden column tiles and runs v_mfma_f32_32x32x2_f32 over the tap's K = C (exact f32);
//   * bias + ReLU -> hidden tile in LDS -> the 1x1 (+ bias) in plain f32, one output per thread -> scatter into the NCHW map.
// Centre points carry three branches (wh, hps, reg): three blocks per centre tile, the same shape as a joint tile.
//
// Determinism: a point's result depends only on its own 3x3 patch -- every output element of an MFMA is its own dot product in a
// fixed k order, and the 1x1 is a per-(point, output) sequential sum -- so a pixel that appears several times (a joint peak of
// two joints, a duplicated index) is written with identical bits by every block that holds it.
#include "common.h"

#define HP_M 32             // points per block (the MFMA's M)

typedef float hp_f32x16 __attribute__((ext_vector_type(16)));

// hidden tiles per wave (the kernels' NS) and the block size of a launch: one wave per NS 32-wide hidden column tiles
static inline int hp_tiles_per_wave(int hc) { return (hc % 64 == 0 && hc >= 128) ? 2 : 1; }
static inline int hp_block_threads(int hc) { return 64 * hc / (32 * hp_tiles_per_wave(hc)); }

// w1: per branch [9C/8][2][hc][4]: element (kb, h, n, s) = weight of hidden channel n at k = 8 kb + 4 h + s (k = tap * C + c);
// lane half h of MFMA step s of k-group kb multiplies A[point][8 kb + 4 h + s] by B[8 kb + 4 h + s][n], so both operands of a
// k-group are one float4 per lane.  b1: [4][hc].  w2: [6 + 2J][hc] rows of wh (2), hps (2J), reg (2), hp_offset (2); b2 alike.
// out: the four NCHW maps [B,n,H,W] back to back in that order (row r of w2 -> map offset r * B * H * W).
template <int NS>
__global__ __launch_bounds__(512) void head_points_kernel(
    const float* __restrict__ feat, int featLd, const int* __restrict__ inds, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
    int B, int H, int W, int C, int J, int K, int hc, int nct)
{
    extern __shared__ __attribute__((aligned(16))) float hp_smem[];
    __shared__ int s_b[HP_M], s_y[HP_M], s_x[HP_M], s_p[HP_M];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x;
    const int HW = H * W, lda = C + 4, ldh = hc + 1;
    float* sA = hp_smem;                          // [HP_M][C + 4]: one tap's gathered rows
    float* sH = hp_smem + HP_M * lda;             // [HP_M][hc + 1]: hidden tile after bias + ReLU

    int br, tile, npts;
    if ((int)blockIdx.x < 3 * nct) { br = blockIdx.x % 3; tile = blockIdx.x / 3; npts = B * K; }
    else { br = 3; tile = blockIdx.x - 3 * nct; npts = B * J * K; }
    const int n_out = (br == 1) ? 2 * J : 2;
    const int row0 = (br == 0) ? 0 : (br == 1) ? 2 : (br == 2) ? 2 + 2 * J : 4 + 2 * J;

    if (tid < HP_M) {
        const int g = tile * HP_M + tid;
        int b = -1, ind = 0;
        if (g < npts) {
            if (br < 3) { b = g / K; ind = inds[((size_t)b * (1 + J)) * K + g % K]; }
            else { b = g / (J * K); const int r = g % (J * K); ind = inds[((size_t)b * (1 + J) + 1 + r / K) * K + r % K]; }
        }
        const int p = ((ind % HW) + HW) % HW;     // decode.py:104 (class plane dropped); joint indices are already in range
        s_b[tid] = b; s_p[tid] = p; s_y[tid] = p / W; s_x[tid] = p % W;
    }

    const float* w1b = w1 + (size_t)br * 9 * C * hc;
    const int r = lane & 31, h = lane >> 5;
    hp_f32x16 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;

    const int c4 = C >> 2;
    for (int tap = 0; tap < 9; ++tap) {
        __syncthreads();                          // point table ready / previous tap's reads of sA done
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        for (int e = tid; e < HP_M * c4; e += nthr) {
            const int i = e / c4, q = e - i * c4;
            const int b = s_b[i], yy = s_y[i] + dy, xx = s_x[i] + dx;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b >= 0 && yy >= 0 && yy < H && xx >= 0 && xx < W)
                v = *reinterpret_cast<const float4*>(feat + ((size_t)(b * H + yy) * W + xx) * featLd + 4 * q);
            *reinterpret_cast<float4*>(sA + i * lda + 4 * q) = v;
        }
        __syncthreads();
        const float* arow = sA + r * lda + 4 * h;
        const float* wt = w1b + (size_t)tap * (C >> 3) * 2 * hc * 4 + ((size_t)h * hc + wid * NS * 32 + r) * 4;
        for (int kb = 0; kb < (C >> 3); ++kb) {
            const float4 a = *reinterpret_cast<const float4*>(arow + 8 * kb);
            float4 bv[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) bv[s] = *reinterpret_cast<const float4*>(wt + (size_t)kb * 2 * hc * 4 + s * 32 * 4);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[s].x, acc[s], 0, 0, 0);
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[s].y, acc[s], 0, 0, 0);
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[s].z, acc[s], 0, 0, 0);
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[s].w, acc[s], 0, 0, 0);
            }
        }
    }

    // bias + ReLU -> hidden tile (C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int n = (wid * NS + s) * 32 + r;
        const float bias = b1[br * hc + n];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
            sH[i * ldh + n] = fmaxf(acc[s][q] + bias, 0.f);
        }
    }
    __syncthreads();

    // 1x1 + bias, one (point, output) per thread, sequential over the hidden channels; scatter into the NCHW map
    float* ob = out + (size_t)row0 * B * HW;
    for (int e = tid; e < HP_M * n_out; e += nthr) {
        const int i = e % HP_M, n = e / HP_M;
        const int b = s_b[i];
        if (b < 0) continue;
        const float* wr = w2 + (size_t)(row0 + n) * hc;
        const float* hr = sH + i * ldh;
        float v = 0.f;
        for (int c = 0; c < hc; ++c) v = fmaf(hr[c], wr[c], v);
        ob[((size_t)b * n_out + n) * HW + s_p[i]] = v + b2[row0 + n];
    }
}

// ---- the same heads under the flip test (multi_pose.py:45-53): N image / mirrored-twin pairs, points of the N MERGED heat maps ----
// feat holds the 2N images with the pairs interleaved (image n at batch 2n, its twin at 2n + 1); inds are the peak extraction's
// [N,1+J,K] on the merged hm / hm_hp.  The decode reads the merged wh / hps / reg / hp_offset at those peaks only, and there
//   wh[c]     = (wh_img[c](y, x) + wh_twin[c](y, W-1-x)) / 2
//   hps[c]    = (hps_img[c](y, x) + sign(c) * hps_twin[2 perm[c >> 1] + (c & 1)](y, W-1-x)) / 2,  sign = -1 for even c (flip_lr_off)
//   reg, hp_offset = the image's own value
// so a reg / hp_offset block is head_points_kernel's block on image 2n, and a wh / hps block runs two passes over the same sA / sH:
// the image at (y, x), whose 1x1 results are parked in LDS ([n_out][32] floats), then the twin at (y, W-1-x) with the twin's own 3x3
// patch and zero padding, whose 1x1 evaluates the twin channel each output merges with.  Each pass keeps head_points_kernel's k order
// (tap, k-group, MFMA step) and its sequential fmaf over the hidden channels, so a side's value is bit for bit what
// cp_head_points_f32 writes for that pixel of that image; the merge is flip_merge_kernel's b = twin * sign, (a + b) / 2.0f.
// out: the four MERGED sparse maps [N,n,H,W] back to back (wh, hps, reg, hp_offset).  No atomics, no dependence between blocks.
template <int NS>
__global__ __launch_bounds__(512) void head_points_pairs_kernel(
    const float* __restrict__ feat, int featLd, const int* __restrict__ inds, const int* __restrict__ perm,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    float* __restrict__ out, int N, int H, int W, int C, int J, int K, int hc, int nct)
{
    extern __shared__ __attribute__((aligned(16))) float hp_smem[];
    __shared__ int s_b[HP_M], s_y[HP_M], s_x[HP_M], s_p[HP_M];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x;
    const int HW = H * W, lda = C + 4, ldh = hc + 1;
    float* sA = hp_smem;                          // [HP_M][C + 4]: one tap's gathered rows
    float* sH = hp_smem + HP_M * lda;             // [HP_M][hc + 1]: hidden tile after bias + ReLU
    float* sP = sH + HP_M * ldh;                  // [2J][HP_M]: the image side's 1x1 results of a wh / hps block

    int br, tile, npts;
    if ((int)blockIdx.x < 3 * nct) { br = blockIdx.x % 3; tile = blockIdx.x / 3; npts = N * K; }
    else { br = 3; tile = blockIdx.x - 3 * nct; npts = N * J * K; }
    const int n_out = (br == 1) ? 2 * J : 2;
    const int row0 = (br == 0) ? 0 : (br == 1) ? 2 : (br == 2) ? 2 + 2 * J : 4 + 2 * J;
    const int nside = br < 2 ? 2 : 1;             // wh, hps: image and twin; reg, hp_offset: the image alone

    if (tid < HP_M) {
        const int g = tile * HP_M + tid;
        int b = -1, ind = 0;                      // b: the PAIR of the point
        if (g < npts) {
            if (br < 3) { b = g / K; ind = inds[((size_t)b * (1 + J)) * K + g % K]; }
            else { b = g / (J * K); const int r = g % (J * K); ind = inds[((size_t)b * (1 + J) + 1 + r / K) * K + r % K]; }
        }
        const int p = ((ind % HW) + HW) % HW;     // decode.py:104 (class plane dropped); joint indices are already in range
        s_b[tid] = b; s_p[tid] = p; s_y[tid] = p / W; s_x[tid] = p % W;
    }

    const float* w1b = w1 + (size_t)br * 9 * C * hc;
    const int r = lane & 31, h = lane >> 5;
    const int c4 = C >> 2;
    float* ob = out + (size_t)row0 * N * HW;

    for (int side = 0; side < nside; ++side) {
        hp_f32x16 acc[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;

        for (int tap = 0; tap < 9; ++tap) {
            __syncthreads();                      // point table ready / previous tap's reads of sA (previous side's of sH) done
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            for (int e = tid; e < HP_M * c4; e += nthr) {
                const int i = e / c4, q = e - i * c4;
                const int b = s_b[i], yy = s_y[i] + dy, xx = (side ? W - 1 - s_x[i] : s_x[i]) + dx;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (b >= 0 && yy >= 0 && yy < H && xx >= 0 && xx < W)
                    v = *reinterpret_cast<const float4*>(feat + ((size_t)((2 * b + side) * H + yy) * W + xx) * featLd + 4 * q);
                *reinterpret_cast<float4*>(sA + i * lda + 4 * q) = v;
            }
            __syncthreads();
            const float* arow = sA + r * lda + 4 * h;
            const float* wt = w1b + (size_t)tap * (C >> 3) * 2 * hc * 4 + ((size_t)h * hc + wid * NS * 32 + r) * 4;
            for (int kb = 0; kb < (C >> 3); ++kb) {
                const float4 a = *reinterpret_cast<const float4*>(arow + 8 * kb);
                float4 bv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) bv[s] = *reinterpret_cast<const float4*>(wt + (size_t)kb * 2 * hc * 4 + s * 32 * 4);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[s].x, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[s].y, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[s].z, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[s].w, acc[s], 0, 0, 0);
                }
            }
        }

        // bias + ReLU -> hidden tile (the previous side's 1x1 reads of sH ended before this side's first tap barrier)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int n = (wid * NS + s) * 32 + r;
            const float bias = b1[br * hc + n];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
                sH[i * ldh + n] = fmaxf(acc[s][q] + bias, 0.f);
            }
        }
        __syncthreads();

        // 1x1 + bias, one (point, output) per thread and the SAME thread on both sides (sP needs no barrier of its own).  The twin
        // side evaluates the twin channel output n merges with, then merges and scatters into the merged NCHW map.
        for (int e = tid; e < HP_M * n_out; e += nthr) {
            const int i = e % HP_M, n = e / HP_M;
            const int b = s_b[i];
            if (b < 0) continue;
            int cs = n;
            float sign = 1.f;
            if (side && br == 1) { cs = 2 * perm[n >> 1] + (n & 1); if ((n & 1) == 0) sign = -1.f; }
            const float* wr = w2 + (size_t)(row0 + cs) * hc;
            const float* hr = sH + i * ldh;
            float v = 0.f;
            for (int c = 0; c < hc; ++c) v = fmaf(hr[c], wr[c], v);
            v += b2[row0 + cs];
            if (nside == 2) {
                if (side == 0) { sP[n * HP_M + i] = v; continue; }
                const float a = sP[n * HP_M + i];
                const float t = v * sign;
                v = (a + t) / 2.0f;
            }
            ob[((size_t)b * n_out + n) * HW + s_p[i]] = v;
        }
    }
}

extern "C" int cp_head_points_f32(const float* feat, int featLd, const int* ws_inds, const float* w1, const float* b1, const float* w2,
                                  const float* b2, float* out, int B, int H, int W, int C, int J, int K, int hc, void* stream)
{
    CP_CHECK_ARG(feat && ws_inds && w1 && b1 && w2 && b2 && out, "head_points: null pointer");
    CP_CHECK_ARG(B > 0 && H > 0 && W > 0 && J > 0 && K > 0 && K <= 256 && K <= (long long)H * W, "head_points: bad shape");
    CP_CHECK_ARG(C > 0 && C % 16 == 0 && C <= 512, "head_points: C=%d must be a multiple of 16 in 16..512 (physical channels)", C);
    CP_CHECK_ARG(featLd >= C && featLd % 4 == 0 && ((size_t)feat & 15) == 0, "head_points: feat must be 16-B aligned with ld %% 4 == 0 (ld %d)", featLd);
    CP_CHECK_ARG(hc > 0 && hc % 32 == 0 && hc <= 512, "head_points: head_conv=%d must be a multiple of 32 up to 512", hc);
    // a wave takes two 32-wide hidden tiles only when hc is a multiple of 64: an odd multiple of 32 above 256 would need 576 .. 960 threads
    CP_CHECK_ARG(hp_block_threads(hc) <= 512, "head_points: head_conv=%d needs a block of %d threads, the kernel takes 512 at most "
                 "(served: multiples of 32 up to 256, multiples of 64 up to 512)", hc, hp_block_threads(hc));
    CP_CHECK_ARG((long long)B * (1 + J) * K < (1ll << 31) && (long long)B * H * W * (6 + 2 * J) < (1ll << 40), "head_points: too large");
    // the kernel keeps H * W, a point's plane index and the pixel row b * H + y in `int`
    CP_CHECK_ARG((long long)H * W < (1ll << 31) && (long long)B * H < (1ll << 31),
                 "head_points: too large: H*W=%lld and B*H=%lld must stay below 2^31 (32-bit plane and row indices)", (long long)H * W, (long long)B * H);
    const int ns = hp_tiles_per_wave(hc);
    const int nthr = hp_block_threads(hc);
    const int nct = cp_cdiv(B * K, HP_M), njt = cp_cdiv(B * J * K, HP_M);
    const size_t lds = (size_t)HP_M * (C + 4) * 4 + (size_t)HP_M * (hc + 1) * 4;
    static CpLdsGuard lds_reserved[2];
    const void* kern = ns == 2 ? (const void*)head_points_kernel<2> : (const void*)head_points_kernel<1>;
    {
        const hipError_t e = lds_reserved[ns - 1].ensure(kern, (int)lds);
        if (e != hipSuccess) { cp_set_error("head_points: cannot reserve %zu B LDS: %s", lds, hipGetErrorString(e)); return 2; }
    }
    hipStream_t s = (hipStream_t)stream;
    if (ns == 2)
        hipLaunchKernelGGL(head_points_kernel<2>, dim3(3 * nct + njt), dim3(nthr), lds, s, feat, featLd, ws_inds, w1, b1, w2, b2, out, B, H, W,
                           C, J, K, hc, nct);
    else
        hipLaunchKernelGGL(head_points_kernel<1>, dim3(3 * nct + njt), dim3(nthr), lds, s, feat, featLd, ws_inds, w1, b1, w2, b2, out, B, H, W,
                           C, J, K, hc, nct);
    CP_CHECK_LAUNCH("head_points_kernel");
    cp_note_kernel(ns == 2 ? "head_points_kernel<2>" : "head_points_kernel<1>");
    return 0;
}

extern "C" int cp_head_points_pairs_f32(const float* feat, int featLd, const int* ws_inds, const int* perm, const float* w1, const float* b1,
                                        const float* w2, const float* b2, float* out, int N, int H, int W, int C, int J, int K, int hc,
                                        void* stream)
{
    CP_CHECK_ARG(feat && ws_inds && w1 && b1 && w2 && b2 && out, "head_points_pairs: null pointer");
    CP_CHECK_ARG(perm, "head_points_pairs: the joint permutation is needed (device int[J])");
    CP_CHECK_ARG(N > 0 && H > 0 && W > 0 && J > 0 && K > 0 && K <= 256 && K <= (long long)H * W, "head_points_pairs: bad shape");
    CP_CHECK_ARG(C > 0 && C % 16 == 0 && C <= 512, "head_points_pairs: C=%d must be a multiple of 16 in 16..512 (physical channels)", C);
    CP_CHECK_ARG(featLd >= C && featLd % 4 == 0 && ((size_t)feat & 15) == 0, "head_points_pairs: feat must be 16-B aligned with ld %% 4 == 0 (ld %d)", featLd);
    CP_CHECK_ARG(hc > 0 && hc % 32 == 0 && hc <= 512, "head_points_pairs: head_conv=%d must be a multiple of 32 up to 512", hc);
    CP_CHECK_ARG(hp_block_threads(hc) <= 512, "head_points_pairs: head_conv=%d needs a block of %d threads, the kernel takes 512 at most "
                 "(served: multiples of 32 up to 256, multiples of 64 up to 512)", hc, hp_block_threads(hc));
    CP_CHECK_ARG((long long)N * (1 + J) * K < (1ll << 31) && (long long)2 * N * H * W * (6 + 2 * J) < (1ll << 40) && (long long)2 * N * H < (1ll << 31),
                 "head_points_pairs: too large");
    CP_CHECK_ARG((long long)H * W < (1ll << 31), "head_points_pairs: too large: H*W=%lld must stay below 2^31 (32-bit plane index)", (long long)H * W);
    const int ns = hp_tiles_per_wave(hc);
    const int nthr = hp_block_threads(hc);
    const int nct = cp_cdiv(N * K, HP_M), njt = cp_cdiv(N * J * K, HP_M);
    const size_t lds = (size_t)HP_M * (C + 4) * 4 + (size_t)HP_M * (hc + 1) * 4 + (size_t)HP_M * 2 * J * 4;
    static CpLdsGuard lds_reserved[2];
    const void* kern = ns == 2 ? (const void*)head_points_pairs_kernel<2> : (const void*)head_points_pairs_kernel<1>;
    {
        const hipError_t e = lds_reserved[ns - 1].ensure(kern, (int)lds);
        if (e != hipSuccess) { cp_set_error("head_points_pairs: cannot reserve %zu B LDS: %s", lds, hipGetErrorString(e)); return 2; }
    }
    hipStream_t s = (hipStream_t)stream;
    if (ns == 2)
        hipLaunchKernelGGL(head_points_pairs_kernel<2>, dim3(3 * nct + njt), dim3(nthr), lds, s, feat, featLd, ws_inds, perm, w1, b1, w2, b2,
                           out, N, H, W, C, J, K, hc, nct);
    else
        hipLaunchKernelGGL(head_points_pairs_kernel<1>, dim3(3 * nct + njt), dim3(nthr), lds, s, feat, featLd, ws_inds, perm, w1, b1, w2, b2,
                           out, N, H, W, C, J, K, hc, nct);
    CP_CHECK_LAUNCH("head_points_pairs_kernel");
    cp_note_kernel(ns == 2 ? "head_points_pairs_kernel<2>" : "head_points_pairs_kernel<1>");
    return 0;
}
