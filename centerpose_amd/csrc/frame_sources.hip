// The batched pre-process of batch_stages.hip for frames that are ALREADY on the device (a video decoder's surface, a data loader's
// CUDA tensor, a planar JPEG decode, a crop of a larger frame): every source is addressed by its own pointer and strides instead of
// one offset into a shared staging buffer, and read in place -- no repack pass, no device-to-device gather.
//
//   cp_preprocess_frames_u8_f32 : cv2.resize + cv2.warpAffine + normalise + HWC->CHW (+ mirrored twin) of base_detector.py:47-58 for N
//                                 frames of any size and layout, one resize launch (when any frame needs it) and one warp launch.
//
// Channel k (network order: cv2's B, G, R) of pixel (y, x) of a frame is the byte at base + y * row_stride + x * pix_stride + ch_off[k]:
// packed BGR, packed RGB (ch_off = {2,1,0}), BGRA / RGBA (pix_stride 4, byte 3 never read), planar CHW (pix_stride 1, ch_off multiples
// of the plane stride), crops, padded rows and expanded (stride 0) views are the same statement.  The arithmetic between the loads is
// pre_arith.h's, shared with batch_stages.hip: results are bit-identical to cp_preprocess_batch_u8_f32 on the equivalent packed BGR
// image.  Compiled with -ffp-contract=off, like batch_stages.hip.
#include <cmath>
#include "common.h"
#include "pre_arith.h"

// mirror of cp_frame_desc (include/centerpose_hip.h)
struct FrameDesc {
    const unsigned char* base;      // device address of pixel (0,0)
    long long row_stride, pix_stride;
    long long ch_off[3];
    long long mid_off;      // byte offset of the resized uint8 [NH,NW,3] image in the scratch buffer, < 0: (NH,NW) == (H,W), no resize
    int H, W, NH, NW;
    double mi[6];           // INVERTED warp matrix: destination pixel -> coordinates in the (resized) image
    int slot, pad;          // output batch index of the image (its mirrored twin goes to slot + 1)
};
static_assert(sizeof(FrameDesc) == 128, "cp_frame_desc is 128 bytes");

// blockIdx.y: frame; blockIdx.x: grid-stride tiles of its resized pixels.  Frames without a resize leave at once.  The intermediate is
// packed [NH,NW,3] in network channel order, whatever the frame's layout.
__global__ __launch_bounds__(BS_THREADS) void resize_frames_u8_kernel(unsigned char* __restrict__ scratch, const FrameDesc* __restrict__ table)
{
    const FrameDesc& d = table[blockIdx.y];
    if (d.mid_off < 0) return;
    const int H = d.H, W = d.W, NH = d.NH, NW = d.NW, total = NH * NW;
    const double scale_x = (double)W / NW, scale_y = (double)H / NH;
    const BsStrided src = {d.base, d.row_stride, d.pix_stride, {d.ch_off[0], d.ch_off[1], d.ch_off[2]}};
    unsigned char* dst = scratch + d.mid_off;
    for (int i = blockIdx.x * BS_THREADS + threadIdx.x; i < total; i += gridDim.x * BS_THREADS) {
        const int dy = i / NW, dx = i - dy * NW;
        bs_resize_pixel(src, H, W, scale_x, scale_y, dx, dy, dst + (size_t)i * 3);
    }
}

// blockIdx.y: frame; blockIdx.x: grid-stride tiles of its OH x OW destination pixels (bs_warp_image, pre_arith.h).  The source is the
// frame itself (no resize) or its packed intermediate: one strided source either way, the choice is uniform over the block.
template <bool VEC>
__global__ __launch_bounds__(BS_THREADS) void preprocess_frames_kernel(const unsigned char* __restrict__ scratch, const FrameDesc* __restrict__ table,
                                                                       float* __restrict__ out, int OH, int OW, BsNorm nm, int flip)
{
    const FrameDesc& d = table[blockIdx.y];
    BsStrided src;
    if (d.mid_off < 0) {
        src.base = d.base; src.row = d.row_stride; src.pix = d.pix_stride;
        src.off[0] = d.ch_off[0]; src.off[1] = d.ch_off[1]; src.off[2] = d.ch_off[2];
    } else {
        src.base = scratch + d.mid_off; src.row = (long long)d.NW * 3; src.pix = 3;
        src.off[0] = 0; src.off[1] = 1; src.off[2] = 2;
    }
    double m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = d.mi[k];
    const size_t total = (size_t)OH * OW;
    float* o = out + (size_t)d.slot * 3 * total;
    bs_warp_image<VEC>(src, d.NH, d.NW, m, o, o + 3 * total, OH, OW, nm, flip);
}

extern "C" int cp_sizeof_frame_desc(void) { return (int)sizeof(FrameDesc); }

// table / table_host: the same N descriptors on the device and on the host (the host copy is what is checked).  The size of a frame's
// allocation is not known here: base, strides and ch_off must describe memory the caller owns (a tensor's own shape / strides do).
extern "C" int cp_preprocess_frames_u8_f32(const void* table, const void* table_host, int N, unsigned char* scratch, size_t scratch_bytes,
                                           float* out, int out_batch, int OH, int OW, const float* mean /* host 3 */,
                                           const float* std_ /* host 3 */, int flip, void* stream)
{
    CP_CHECK_ARG(table && table_host && out && mean && std_ && N > 0 && OH > 0 && OW > 0 && out_batch > 0, "preprocess_frames: bad arguments");
    CP_CHECK_ARG(N <= 65535, "preprocess_frames: at most 65535 frames per launch (got %d)", N);
    CP_CHECK_ARG((long long)OH * OW < (1ll << 29), "preprocess_frames: output %d x %d too large", OH, OW);
    const FrameDesc* th = (const FrameDesc*)table_host;
    const int nb = flip ? 2 : 1;
    long long max_resized = 0;
    for (int n = 0; n < N; ++n) {
        const FrameDesc& d = th[n];
        CP_CHECK_ARG(d.base, "preprocess_frames: frame %d: null base address", n);
        CP_CHECK_ARG(d.H > 0 && d.W > 0 && d.NH > 0 && d.NW > 0 && (long long)d.H * d.W < (1ll << 29) && (long long)d.NH * d.NW < (1ll << 29),
                     "preprocess_frames: frame %d: bad size %d x %d -> %d x %d", n, d.H, d.W, d.NH, d.NW);
        CP_CHECK_ARG(d.row_stride >= 0 && d.pix_stride >= 0 && d.ch_off[0] >= 0 && d.ch_off[1] >= 0 && d.ch_off[2] >= 0,
                     "preprocess_frames: frame %d: negative stride or channel offset", n);
        long long ch_max = d.ch_off[0];
        if (d.ch_off[1] > ch_max) ch_max = d.ch_off[1];
        if (d.ch_off[2] > ch_max) ch_max = d.ch_off[2];
        const __int128 last = (__int128)(d.H - 1) * d.row_stride + (__int128)(d.W - 1) * d.pix_stride + ch_max;
        CP_CHECK_ARG(last < ((__int128)1 << 62), "preprocess_frames: frame %d: strides address more than 2^62 bytes", n);
        const long long mid_bytes = (long long)d.NH * d.NW * 3;
        if (d.mid_off >= 0) {
            CP_CHECK_ARG(scratch && d.mid_off + mid_bytes <= (long long)scratch_bytes, "preprocess_frames: frame %d: resized image lies outside the scratch buffer", n);
            if ((long long)d.NH * d.NW > max_resized) max_resized = (long long)d.NH * d.NW;
        } else {
            CP_CHECK_ARG(d.NH == d.H && d.NW == d.W, "preprocess_frames: frame %d: %d x %d -> %d x %d needs a scratch offset", n, d.H, d.W, d.NH, d.NW);
        }
        CP_CHECK_ARG(d.slot >= 0 && d.slot + nb <= out_batch, "preprocess_frames: frame %d: output slot %d outside the batch of %d", n, d.slot, out_batch);
    }
    hipStream_t s = (hipStream_t)stream;
    if (max_resized > 0) {
        long long gx = (max_resized + BS_THREADS - 1) / BS_THREADS;
        if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(resize_frames_u8_kernel, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, scratch, (const FrameDesc*)table);
        CP_CHECK_LAUNCH("resize_frames_u8_kernel");
    }
    BsNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.sd[c] = std_[c]; }
    const bool vec = OW % 4 == 0 && ((size_t)out & 15) == 0;
    long long gx = ((long long)OH * (vec ? OW / 4 : OW) + BS_THREADS - 1) / BS_THREADS;
    if (gx > 4096) gx = 4096;
    if (vec)
        hipLaunchKernelGGL(preprocess_frames_kernel<true>, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, scratch,
                           (const FrameDesc*)table, out, OH, OW, nm, flip ? 1 : 0);
    else
        hipLaunchKernelGGL(preprocess_frames_kernel<false>, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, scratch,
                           (const FrameDesc*)table, out, OH, OW, nm, flip ? 1 : 0);
    CP_CHECK_LAUNCH("preprocess_frames_kernel");
    cp_note_kernel(vec ? "preprocess_frames_kernel<vec4>" : "preprocess_frames_kernel<scalar>");
    return 0;
}
