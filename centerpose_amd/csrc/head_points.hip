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

extern "C" int cp_head_points_f32(const float* feat, int featLd, const int* ws_inds, const float* w1, const float* b1, const float* w2,
                                  const float* b2, float* out, int B, int H, int W, int C, int J, int K, int hc, void* stream)
{
    CP_CHECK_ARG(feat && ws_inds && w1 && b1 && w2 && b2 && out, "head_points: null pointer");
    CP_CHECK_ARG(B > 0 && H > 0 && W > 0 && J > 0 && K > 0 && K <= 256 && K <= H * W, "head_points: bad shape");
    CP_CHECK_ARG(C > 0 && C % 16 == 0 && C <= 512, "head_points: C=%d must be a multiple of 16 in 16..512 (physical channels)", C);
    CP_CHECK_ARG(featLd >= C && featLd % 4 == 0 && ((size_t)feat & 15) == 0, "head_points: feat must be 16-B aligned with ld %% 4 == 0 (ld %d)", featLd);
    CP_CHECK_ARG(hc > 0 && hc % 32 == 0 && hc <= 512, "head_points: head_conv=%d must be a multiple of 32 up to 512", hc);
    CP_CHECK_ARG((long long)B * (1 + J) * K < (1ll << 31) && (long long)B * H * W * (6 + 2 * J) < (1ll << 40), "head_points: too large");
    const int ns = (hc % 64 == 0 && hc >= 128) ? 2 : 1;
    const int nthr = 64 * hc / (32 * ns);
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
