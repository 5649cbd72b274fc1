// Batched flip-test merge on gfx950 (multi_pose.py:45-53; models/utils.py:27-47) for N image / mirrored-twin pairs at once.
// Input maps are NCHW [2N, C, H, W] with the pairs interleaved: image n at batch 2n, its twin at 2n + 1 (torch.cat of N
// pre_process outputs).  Output maps are [N, C, H, W].  Per map a mode:
//   0: hm, wh            out = (in[2n] + flip_w(in[2n+1])) / 2
//   1: hm_hp             the twin's channels through the left/right joint permutation first
//   2: hps               the swap on (x, y) pairs, x components negated (flip_lr_off)
//   3: reg, hp_offset    out = in[2n] (the reference keeps the image's own map: reg[0:1], hp_offset[0:1])
// The arithmetic is that of flip_merge_kernel (elementwise.hip): b = twin * sign, (a + b) / 2.0f in f32 -- bit for bit the same
// results.  Up to four maps per launch: each owns a contiguous range of blocks, selected with a scalar loop as in
// sum_up_group_kernel.  HBM-bound: with W % 4 == 0 and 16-B aligned maps every lane moves 4 consecutive x -- the image row as one
// float4, the mirrored span (also 16-B aligned then: W - 4 - x0 is a multiple of 4) as one float4 with its lanes reversed.
#include "common.h"

#define FP_THREADS 256

struct FlipPairsMap { const float* in; float* out; int C, mode, blocks0; };
struct FlipPairsArgs { FlipPairsMap m[4]; int n, N, H, W; const int* perm; };

template <bool VEC>
__global__ __launch_bounds__(FP_THREADS) void flip_merge_pairs_kernel(const FlipPairsArgs a)
{
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.m[k + 1].blocks0) ++k;        // scalar
    const FlipPairsMap& m = a.m[k];
    const int H = a.H, W = a.W, C = m.C, mode = m.mode;
    const int Wq = VEC ? W >> 2 : W;                                         // work items per row
    const int t = ((int)blockIdx.x - m.blocks0) * FP_THREADS + (int)threadIdx.x;
    if (t >= a.N * C * H * Wq) return;
    const int xq = t % Wq;
    int r = t / Wq;
    const int y = r % H;
    r /= H;
    const int c = r % C, n = r / C;
    const size_t HW = (size_t)H * W, plane = (size_t)C * HW;
    const float* img = m.in + 2 * (size_t)n * plane + (size_t)c * HW + (size_t)y * W;
    float* o = m.out + (size_t)n * plane + (size_t)c * HW + (size_t)y * W;
    if (mode == 3) {
        if (VEC) *reinterpret_cast<float4*>(o + 4 * xq) = *reinterpret_cast<const float4*>(img + 4 * xq);
        else o[xq] = img[xq];
        return;
    }
    int cs = c;
    float sign = 1.f;
    if (mode == 1) cs = a.perm[c];
    else if (mode == 2) { cs = 2 * a.perm[c >> 1] + (c & 1); if ((c & 1) == 0) sign = -1.f; }
    const float* twin = m.in + (2 * (size_t)n + 1) * plane + (size_t)cs * HW + (size_t)y * W;
    if (VEC) {
        const int x0 = 4 * xq;
        const float4 va = *reinterpret_cast<const float4*>(img + x0);
        const float4 vb = *reinterpret_cast<const float4*>(twin + (W - 4 - x0));       // x0 + i <- W - 1 - x0 - i: lanes reversed
        const float b0 = vb.w * sign, b1 = vb.z * sign, b2 = vb.y * sign, b3 = vb.x * sign;
        *reinterpret_cast<float4*>(o + x0) = make_float4((va.x + b0) / 2.0f, (va.y + b1) / 2.0f, (va.z + b2) / 2.0f, (va.w + b3) / 2.0f);
    } else {
        const float b = twin[W - 1 - xq] * sign;
        o[xq] = (img[xq] + b) / 2.0f;
    }
}

// n <= 4 maps; in / out: n pointers each; meta: [n][2] = C, mode; perm: DEVICE int32 [J] (modes 1 and 2), J joints.
extern "C" int cp_flip_merge_pairs_f32(int n, const float* const* in, float* const* out, const int* meta, int N, int H, int W, int J,
                                       const int* perm, void* stream)
{
    CP_CHECK_ARG(n >= 1 && n <= 4 && in && out && meta, "flip_merge_pairs: 1..4 maps (got %d)", n);
    CP_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "flip_merge_pairs: bad shape N=%d H=%d W=%d", N, H, W);
    FlipPairsArgs a;
    a.n = n; a.N = N; a.H = H; a.W = W; a.perm = perm;
    bool vec = W % 4 == 0;
    for (int k = 0; k < n; ++k) {
        const int C = meta[2 * k], mode = meta[2 * k + 1];
        CP_CHECK_ARG(in[k] && out[k] && C >= 1 && mode >= 0 && mode <= 3, "flip_merge_pairs: map %d: bad arguments (C=%d mode=%d)", k, C, mode);
        CP_CHECK_ARG(mode == 0 || mode == 3 || (perm && J >= 1 && C == (mode == 1 ? J : 2 * J)),
                     "flip_merge_pairs: map %d: mode %d needs the joint permutation and %d channels (J=%d), got %d", k, mode,
                     mode == 1 ? J : 2 * J, J, C);
        CP_CHECK_ARG((long long)N * C * H * W < (1ll << 31), "flip_merge_pairs: map %d too large", k);
        vec = vec && ((size_t)in[k] & 15) == 0 && ((size_t)out[k] & 15) == 0;
    }
    long long blocks = 0;
    for (int k = 0; k < 4; ++k) {
        const int kk = k < n ? k : 0;                                        // unused slots repeat map 0 (never selected)
        a.m[k].in = in[kk]; a.m[k].out = out[kk]; a.m[k].C = meta[2 * kk]; a.m[k].mode = meta[2 * kk + 1];
        a.m[k].blocks0 = (int)blocks;
        if (k < n) blocks += ((long long)N * a.m[k].C * H * (vec ? W / 4 : W) + FP_THREADS - 1) / FP_THREADS;
    }
    CP_CHECK_ARG(blocks < (1ll << 31), "flip_merge_pairs: too many blocks");
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(flip_merge_pairs_kernel<true>, dim3((unsigned)blocks), dim3(FP_THREADS), 0, s, a);
    else hipLaunchKernelGGL(flip_merge_pairs_kernel<false>, dim3((unsigned)blocks), dim3(FP_THREADS), 0, s, a);
    CP_CHECK_LAUNCH("flip_merge_pairs_kernel");
    cp_note_kernel(vec ? "flip_merge_pairs_kernel<vec4>" : "flip_merge_pairs_kernel<scalar>");
    return 0;
}
