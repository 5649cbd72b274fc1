// The batched pre-process of frame_sources.hip for device frames in 4:2:0 YUV (a hardware decoder's NV12 surface, NV21, I420 / YV12):
// the (Y, U, V) samples are turned into the B, G, R bytes at the point where the taps are loaded, so no BGR copy of a frame is ever
// written and no conversion launch runs before the pre-process.
//
//   cp_preprocess_yuv_frames_u8_f32 : cv2.resize + cv2.warpAffine + normalise + HWC->CHW (+ mirrored twin) of the BGR image a frame
//                                     converts to, for N frames of any size and plane layout: one resize launch (when any frame needs
//                                     it) and one warp launch.
//   cp_yuv_to_bgr_host              : the conversion of n (Y, U, V) triples on the CPU, by the same statements.
//
// Y(r, c) is the byte at y_base + r * y_row + c * y_pix, U(r, c) the byte at u_base + (r >> 1) * c_row + (c >> 1) * c_pix, V(r, c) the
// same expression from v_base: nearest chroma, one pair per 2x2 block.  NV12: v_base = u_base + 1, c_pix = 2; NV21: u_base = v_base + 1;
// I420 / YV12: two planes, c_pix = 1; pitched rows, crops at even origins and expanded (stride 0) planes are the same rule.  The
// conversion is yuv_arith.h's (integer, per source pixel, before the resize and before the warp); everything after the load is
// pre_arith.h's, shared with batch_stages.hip and frame_sources.hip: results are bit-identical to cp_preprocess_frames_u8_f32 on the
// packed BGR image obtained by converting every pixel.  Compiled with -ffp-contract=off, like frame_sources.hip.
//
// That is format word 0 of a descriptor.  Any other word (yuv_source.h: 4:2:2 / 4:4:4 chroma, 16-bit samples as in P010 / P016, grey)
// sends the whole launch through the general instantiations, reported as preprocess_yuv_surfaces_kernel<vec4|scalar>; the conversion
// of 16-bit samples is yf_yuv16_to_bgr, on the CPU through cp_yuv16_to_bgr_host.
#include <cmath>
#include "common.h"
#include "pre_arith.h"
#include "yuv_source.h"

// mirror of cp_yuv_frame_desc (include/centerpose_hip.h)
struct YuvFrameDesc {
    const unsigned char* y_base;    // device address of Y(0,0)
    long long y_row, y_pix;
    const unsigned char* u_base;    // device addresses of U(0,0), V(0,0)
    const unsigned char* v_base;
    long long c_row, c_pix;         // strides of both chroma planes, per chroma sample
    long long mid_off;      // byte offset of the resized uint8 [NH,NW,3] BGR image in the scratch buffer, < 0: (NH,NW) == (H,W), no resize
    int H, W, NH, NW;
    double mi[6];           // INVERTED warp matrix: destination pixel -> coordinates in the (resized) image
    int slot, pad;          // output batch index of the image (its mirrored twin goes to slot + 1); pad: the format word (yuv_source.h)
};
static_assert(sizeof(YuvFrameDesc) == 136, "cp_yuv_frame_desc is 136 bytes");

// A YUV frame as a source of pre_arith.h is yuv_source.h's YsSource: load(y, x, v) converts the samples of pixel (y, x) to its B, G, R
// bytes.  GEN = false: 8-bit 4:2:0 (every frame of the launch has format word 0), three byte loads per tap, whatever the plane layout.
// Two refinements were measured on the device and are NOT there, because both made the launches slower: one
// 2-byte load for an interleaved pair at an even address, and keeping a lane's last chroma pairs for the neighbouring taps.
// GEN = true: any format word, read per frame (uniform over a block): 4:2:2 / 4:4:4 / grey, 16-bit samples by one 2-byte load each.

// blockIdx.y: frame; blockIdx.x: grid-stride tiles of its resized pixels.  Frames without a resize leave at once.  The intermediate is
// packed [NH,NW,3] BGR, whatever the frame's plane layout.
template <bool GEN>
__global__ __launch_bounds__(BS_THREADS) void resize_yuv_frames_u8_kernel(unsigned char* __restrict__ scratch, const YuvFrameDesc* __restrict__ table,
                                                                          YfCoef coef)
{
    const YuvFrameDesc& d = table[blockIdx.y];
    if (d.mid_off < 0) return;
    const int H = d.H, W = d.W, NH = d.NH, NW = d.NW, total = NH * NW;
    const double scale_x = (double)W / NW, scale_y = (double)H / NH;
    const YsSource<GEN> src = ys_source<GEN>(d, coef);
    unsigned char* dst = scratch + d.mid_off;
    for (int i = blockIdx.x * BS_THREADS + threadIdx.x; i < total; i += gridDim.x * BS_THREADS) {
        const int dy = i / NW, dx = i - dy * NW;
        bs_resize_pixel(src, H, W, scale_x, scale_y, dx, dy, dst + (size_t)i * 3);
    }
}

// blockIdx.y: frame; blockIdx.x: grid-stride tiles of its OH x OW destination pixels (bs_warp_image, pre_arith.h).  The source is the
// frame itself, converted tap by tap (no resize), or its packed BGR intermediate; the choice is uniform over the block.
template <bool VEC, bool GEN>
__global__ __launch_bounds__(BS_THREADS) void preprocess_yuv_frames_kernel(const unsigned char* __restrict__ scratch, const YuvFrameDesc* __restrict__ table,
                                                                           YfCoef coef, float* __restrict__ out, int OH, int OW, BsNorm nm, int flip)
{
    const YuvFrameDesc& d = table[blockIdx.y];
    double m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = d.mi[k];
    const size_t total = (size_t)OH * OW;
    float* o = out + (size_t)d.slot * 3 * total;
    if (d.mid_off < 0) {
        const YsSource<GEN> src = ys_source<GEN>(d, coef);
        bs_warp_image<VEC>(src, d.NH, d.NW, m, o, o + 3 * total, OH, OW, nm, flip);
    } else {
        const BsPacked src = {scratch + d.mid_off, d.NW};
        bs_warp_image<VEC>(src, d.NH, d.NW, m, o, o + 3 * total, OH, OW, nm, flip);
    }
}

extern "C" int cp_sizeof_yuv_frame_desc(void) { return (int)sizeof(YuvFrameDesc); }

static int yf_check_coef(const int* coef, const char* who, YfCoef* k)
{
    const char* why = "";
    CP_CHECK_ARG(coef, "%s: null coef", who);
    CP_CHECK_ARG(yf_coef_fits(coef, &why), "%s: coef (%d, %d, %d, %d, %d, %d): %s", who, coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], why);
    *k = YfCoef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    return 0;
}

// n (Y, U, V) triples -> bgr[3 * n] on the HOST, by yf_yuv_to_bgr: the statements the kernels compile
extern "C" int cp_yuv_to_bgr_host(const unsigned char* y, const unsigned char* u, const unsigned char* v, size_t n, const int* coef,
                                  unsigned char* bgr)
{
    CP_CHECK_ARG(y && u && v && bgr, "yuv_to_bgr_host: null pointer");
    YfCoef k;
    if (int rc = yf_check_coef(coef, "yuv_to_bgr_host", &k)) return rc;
    for (size_t i = 0; i < n; ++i) {
        int p[3];
        yf_yuv_to_bgr(y[i], u[i], v[i], k, p);
        bgr[3 * i] = (unsigned char)p[0]; bgr[3 * i + 1] = (unsigned char)p[1]; bgr[3 * i + 2] = (unsigned char)p[2];
    }
    return 0;
}

// the same for n triples of 16-bit container values, by yf_yuv16_to_bgr
extern "C" int cp_yuv16_to_bgr_host(const unsigned short* y, const unsigned short* u, const unsigned short* v, size_t n, const int* coef,
                                    unsigned char* bgr)
{
    CP_CHECK_ARG(y && u && v && bgr, "yuv16_to_bgr_host: null pointer");
    YfCoef k;
    if (int rc = yf_check_coef(coef, "yuv16_to_bgr_host", &k)) return rc;
    for (size_t i = 0; i < n; ++i) {
        int p[3];
        yf_yuv16_to_bgr(y[i], u[i], v[i], k, p);
        bgr[3 * i] = (unsigned char)p[0]; bgr[3 * i + 1] = (unsigned char)p[1]; bgr[3 * i + 2] = (unsigned char)p[2];
    }
    return 0;
}

template <bool GEN>
static int yf_launch(const YuvFrameDesc* table, int N, const YfCoef& k, unsigned char* scratch, long long max_resized, float* out, int OH, int OW,
                     const BsNorm& nm, int flip, bool vec, hipStream_t s)
{
    if (max_resized > 0) {
        long long gx = (max_resized + BS_THREADS - 1) / BS_THREADS;
        if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(resize_yuv_frames_u8_kernel<GEN>, dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, scratch, table, k);
        CP_CHECK_LAUNCH(GEN ? "resize_yuv_surfaces_u8_kernel" : "resize_yuv_frames_u8_kernel");
    }
    long long gx = ((long long)OH * (vec ? OW / 4 : OW) + BS_THREADS - 1) / BS_THREADS;
    if (gx > 4096) gx = 4096;
    if (vec)
        hipLaunchKernelGGL((preprocess_yuv_frames_kernel<true, GEN>), dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, scratch, table, k, out,
                           OH, OW, nm, flip ? 1 : 0);
    else
        hipLaunchKernelGGL((preprocess_yuv_frames_kernel<false, GEN>), dim3((unsigned)gx, (unsigned)N), dim3(BS_THREADS), 0, s, scratch, table, k, out,
                           OH, OW, nm, flip ? 1 : 0);
    CP_CHECK_LAUNCH(GEN ? "preprocess_yuv_surfaces_kernel" : "preprocess_yuv_frames_kernel");
    return 0;
}

// table / table_host: the same N descriptors on the device and on the host (the host copy is what is checked).  The size of a plane's
// allocation is not known here: bases and strides must describe memory the caller owns (a tensor's own shape / strides do).
extern "C" int cp_preprocess_yuv_frames_u8_f32(const void* table, const void* table_host, int N, const int* coef /* host 6 */,
                                               unsigned char* scratch, size_t scratch_bytes, float* out, int out_batch, int OH, int OW,
                                               const float* mean /* host 3 */, const float* std_ /* host 3 */, int flip, void* stream)
{
    CP_CHECK_ARG(table && table_host && out && mean && std_ && N > 0 && OH > 0 && OW > 0 && out_batch > 0, "preprocess_yuv_frames: bad arguments");
    CP_CHECK_ARG(N <= 65535, "preprocess_yuv_frames: at most 65535 frames per launch (got %d)", N);
    CP_CHECK_ARG((long long)OH * OW < (1ll << 29), "preprocess_yuv_frames: output %d x %d too large", OH, OW);
    YfCoef k;
    if (int rc = yf_check_coef(coef, "preprocess_yuv_frames", &k)) return rc;
    const YuvFrameDesc* th = (const YuvFrameDesc*)table_host;
    const int nb = flip ? 2 : 1;
    long long max_resized = 0;
    bool general = false;
    for (int n = 0; n < N; ++n) {
        const YuvFrameDesc& d = th[n];
        CP_CHECK_ARG(d.H > 0 && d.W > 0 && d.NH > 0 && d.NW > 0 && (long long)d.H * d.W < (1ll << 29) && (long long)d.NH * d.NW < (1ll << 29),
                     "preprocess_yuv_frames: frame %d: bad size %d x %d -> %d x %d", n, d.H, d.W, d.NH, d.NW);
        const char* bad = ys_check_format(d);
        CP_CHECK_ARG(!bad, "preprocess_yuv_frames: frame %d: %s (format word pad = %d; y %p, u %p, v %p)", n, bad, d.pad, (const void*)d.y_base,
                     (const void*)d.u_base, (const void*)d.v_base);
        general = general || d.pad != 0;
        const long long mid_bytes = (long long)d.NH * d.NW * 3;
        if (d.mid_off >= 0) {
            CP_CHECK_ARG(scratch && d.mid_off + mid_bytes <= (long long)scratch_bytes, "preprocess_yuv_frames: frame %d: resized image lies outside the scratch buffer", n);
            if ((long long)d.NH * d.NW > max_resized) max_resized = (long long)d.NH * d.NW;
        } else {
            CP_CHECK_ARG(d.NH == d.H && d.NW == d.W, "preprocess_yuv_frames: frame %d: %d x %d -> %d x %d needs a scratch offset", n, d.H, d.W, d.NH, d.NW);
        }
        CP_CHECK_ARG(d.slot >= 0 && d.slot + nb <= out_batch, "preprocess_yuv_frames: frame %d: output slot %d outside the batch of %d", n, d.slot, out_batch);
    }
    BsNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.sd[c] = std_[c]; }
    const bool vec = OW % 4 == 0 && ((size_t)out & 15) == 0;
    // every frame 8-bit 4:2:0: the kernels as they were before the format word; else ONE general pair for all frames of the launch
    if (int rc = general ? yf_launch<true>((const YuvFrameDesc*)table, N, k, scratch, max_resized, out, OH, OW, nm, flip, vec, (hipStream_t)stream)
                         : yf_launch<false>((const YuvFrameDesc*)table, N, k, scratch, max_resized, out, OH, OW, nm, flip, vec, (hipStream_t)stream))
        return rc;
    if (general)
        cp_note_kernel(vec ? "preprocess_yuv_surfaces_kernel<vec4>" : "preprocess_yuv_surfaces_kernel<scalar>");
    else
        cp_note_kernel(vec ? "preprocess_yuv_frames_kernel<vec4>" : "preprocess_yuv_frames_kernel<scalar>");
    return 0;
}
