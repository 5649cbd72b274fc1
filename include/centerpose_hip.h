/* centerpose_hip.h -- C ABI of libcenterpose_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the inference hot path of tensorboy/centerpose.  Plain pointers and
 * sizes, no torch types.  All pointers are DEVICE pointers unless stated; `stream` is a
 * hipStream_t (NULL = default stream).  Every function returns 0 on success, non-zero on error
 * (1 = bad argument, 2 = launch/runtime failure); cp_last_error() gives the message
 * (thread-local).  The kernel entry points never synchronise the host and never allocate device memory; kernels
 * are enqueued on `stream` only (so a caller may capture a sequence of calls into a hipGraph).  The plan handle
 * (cp_plan_*) is the one exception and says so.
 * Source images reach the pre-process either through one staging buffer (cp_pre_desc) or, when they are on the device already, in
 * place through a per-frame address and strides (cp_frame_desc; cp_yuv_frame_desc for 4:2:0 YUV planes, converted to BGR where the
 * pixels are loaded); all are read when `stream` reaches the launches.
 *
 * File:line citations are relative to the reference checkout (/root/reference).
 * Activation layout: NHWC float32, `ld` = floats between consecutive pixels (>= C).
 */
#ifndef CENTERPOSE_HIP_H
#define CENTERPOSE_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

int cp_abi_version(void);
const char* cp_target_arch(void);            /* "gfx950" */
const char* cp_last_error(void);
const char* cp_last_kernel(void);            /* device kernel (template instantiation) the calling thread launched last */

enum { CP_ACT_NONE = 0, CP_ACT_RELU = 1, CP_ACT_SIGMOID = 2,
       CP_ACT_HSWISH = 3, CP_ACT_HSIGMOID = 4 };   /* x*relu6(x+3)/6, relu6(x+3)/6: lib/models/backbones/mobilenet/mobilenetv3.py:87-96 */

/* ---- fused convolution (implicit GEMM, fp32 MFMA) ------------------------------------------------
 * Replaces nn.Conv2d + BatchNorm2d(eval) + ReLU + residual add + torch.cat (+ sigmoid) of
 *   lib/models/backbones/pose_dla_dcn.py:29-57,145-163,272-282 (BasicBlock, Root, conv levels),
 *   lib/models/backbones/msra_resnet.py:64-102,168-193 (Bottleneck, dense ConvTranspose2d k4 s2 p1 as
 *   4 sub-pixel 2x2 convs via the osy/osx/ooy/oox output scatter),
 *   lib/models/backbones/pose_higher_hrnet.py:98-235, lib/models/heads/keypoint.py:14-42,
 *   and the in-place sigmoid of lib/detectors/multi_pose.py:35-37.
 * out = act( (sum over up to 4 channel-concatenated sources of conv(src)) * scale + shift [+ res] ).
 * w: packed weights [ldw][K] (n-major, k contiguous), k = (ky*kw + kx)*Ctot + c  (inNCHW stem:
 * k = (c*kh + ky)*kw + kx, K padded to a multiple of 16 with zeros), ldw = Cout padded to 16 / 32 / a
 * multiple of 64 with zero rows;  3x3/s1/p1 single-source NHWC launches use the LDS halo-patch kernel;
 * scale/shift: [ldw] (folded BN or 1/bias).  res: NHWC residual with pixel stride resLd, or NULL.
 * Size limits (32-bit device offsets; a larger problem is refused with rc 1): B*H*W < 2^31, B*Ho*Wo + 255 < 2^31, per NHWC source
 * B*H*W*srcLd*4 < 2^32 bytes, and for the inNCHW source B*srcC[0]*H*W < 2^31 floats. */
typedef struct cp_conv_desc {
    int nsrc;                 /* 1..4 sources */
    int srcC[4], srcLd[4];    /* channels taken from / pixel stride of each source (C % 16 == 0 unless inNCHW) */
    int B, H, W;              /* input spatial size */
    int Ho, Wo;               /* output positions computed by this launch */
    int kh, kw, sy, sx, py, px;
    int K, ldw;
    int Cout;                 /* channels stored */
    int resLd, outLd;
    int outNCHW;              /* 0: out is NHWC [B,OH,OW,outLd]; 1: out is NCHW [B,Cout,OH,OW] */
    int OH, OW, osy, osx, ooy, oox;   /* output pixel = (oy*osy+ooy, ox*osx+oox) inside [OH,OW] */
    int act;
    int inNCHW;               /* 1: src[0] is the NCHW network input [B,srcC[0],H,W] (base_detector.py:53-58) */
    int tile;                 /* 0 = auto; BM*1000+BN to force a kernel instantiation; 3000000 + BM*1000 + BN (BM, BN in {128, 64}): the
                                 OPT-IN split-bf16 kernel below -- `w` is then cp_split_bf16_weights_f32's output, NHWC sources only */
    int nsub;                 /* 0 / 1: one convolution.  4: the four sub-pixel 2x2 convolutions of a dense ConvTranspose2d(k4,s2,p1)
                                 (msra_resnet.py:168-193) in ONE launch: w = [4][ldw][K] (sub g = py*2+px), py = px = 1, osy = osx = 2,
                                 ooy = oox = 0; sub g uses pad (1-py, 1-px) and output phase (py, px) */
    int ksplit;               /* 0 / 1: none.  S > 1: split over the reduction axis for launches too small to fill the chip -- over the
                                 input channels (cp_conv3x3_winograd_f32) or the k-steps (cp_conv2d_f32: one NHWC source, nsub = 1, dense
                                 NHWC output): `out` is a workspace [S][B*Ho*Wo][outLd] of raw partial outputs (scale = ones, shift =
                                 zeros, act = CP_ACT_NONE, no residual); cp_splitk_reduce_f32 (ldw = outLd) finishes the layer */
} cp_conv_desc;
int cp_conv2d_f32(const cp_conv_desc* d, const float* const* src, const float* w, const float* scale, const float* shift,
                  const float* res, float* out, void* stream);

/* Up to 8 INDEPENDENT convolutions of the cp_conv2d_f32 kind in ONE launch: the fuse layers of an HRNet module
 * (pose_higher_hrnet.py:169-212: the 1x1 convs of the up paths and the stride-2 3x3 convs of the down paths read only the branch
 * outputs, 16-256 blocks each).  d[i], src[i], w[i], scale[i], shift[i], res[i] (may be NULL), out[i]: member i as for
 * cp_conv2d_f32 with nsrc = 1, NHWC in / dense NHWC out, ldw % 64 == 0, nsub <= 1, ksplit <= 1; outputs must not alias. */
int cp_conv2d_group_f32(const cp_conv_desc* d, int n, const float* const* src, const float* const* w, const float* const* scale,
                        const float* const* shift, const float* const* res, float* const* out, void* stream);

/* Opt-in fp32-EQUIVALENT mode of cp_conv2d_f32 on the bf16 matrix pipe (conv_igemm_bf16x3.hip; never the default, the reference's
 * arithmetic is fp32 end to end: DCNv2/src/cuda/dcn_v2_cuda.cu:58): every fp32 operand is three bf16 terms (8+8+8 significand bits,
 * exact), six bf16 MFMAs with fp32 accumulate per product tile, dropped terms <= 2^-24 relative.  Activations are split in the
 * kernel; weights once, here: w [rows][K] (rows = nsub * ldw, the layout cp_conv2d_f32 takes) -> wb, cp_split_bf16_weight_floats
 * (rows, K) floats holding bf16 [nsub][K/16][ldw][3][16].  Pass wb as `w` together with tile = 3128128 / 3064128 (ldw % 128 == 0) / 3128064 / 3064064. */
size_t cp_split_bf16_weight_floats(int rows, int K);
int cp_split_bf16_weights_f32(const float* w, int rows, int ldw, int K, float* wb, void* stream);

/* ---- 3x3 / stride 1 / pad 1 convolution as fused Winograd F(2x2,3x3) ---------------------------------
 * Same layers and epilogue as cp_conv2d_f32 (the reference gets these from cuDNN, which chooses the algorithm itself --
 * heuristics, or autotuned with CUDNN.BENCHMARK, lib/config/default.py:29, tools/train.py:32); 16 multiplies per
 * 2x2 output tile and (cin, cout) instead of 36, fp32 throughout (error ~3e-6 relative, below the direct kernel's).
 * cp_winograd_pack_f32: packed direct weights w [rows >= Cout][9*C] (k = (ky*3+kx)*C + c, as for cp_conv2d_f32)
 *   -> u [cp_winograd_weight_floats(C, Cout)] = G g G^T in the kernel's MFMA B-fragment order; C % 16 == 0.
 * cp_conv3x3_winograd_f32: d as for cp_conv2d_f32 with nsrc = 1, kh = kw = 3, stride 1, pad 1, NHWC in/out
 *   (returns 1 for any other shape); d->tile: 0 = auto, MT*10+NT in {11, 12, 21} forces a block shape, 64xx the
 *   V-stationary kernel for 64 input channels with xx channel-tile groups per spatial tile; 24 = the F(2x4,3x3) kernel
 *   (conv3x3_wino24.hip: 2x4 output tiles, 24 multiplies per tile and (cin, cout) = 3 per output instead of 4; `u` must then
 *   come from cp_winograd24_pack_f32 -- same argument meaning, [cp_winograd24_weight_floats(C, Cout)] floats; no split-C). */
size_t cp_winograd_weight_floats(int C, int Cout);
int cp_winograd_pack_f32(const float* w, float* u, int C, int Cout, void* stream);
size_t cp_winograd24_weight_floats(int C, int Cout);
int cp_winograd24_pack_f32(const float* w, float* u, int C, int Cout, void* stream);
int cp_conv3x3_winograd_f32(const cp_conv_desc* d, const float* src, const float* u, const float* scale, const float* shift,
                            const float* res, float* out, void* stream);

/* Up to four INDEPENDENT 3x3 / stride-1 / pad-1 convolutions on the F(2x4,3x3) kernel in ONE launch -- the same convolution of every parallel
 * HRNet branch (pose_higher_hrnet.py:217-235): launched one by one, the low-resolution branches leave most CUs idle.  Member i = (d[i], src[i],
 * u[i] from cp_winograd24_pack_f32, scale[i], shift[i], res[i] or NULL, out[i]) as for cp_conv3x3_winograd_f32; outputs must not alias. */
int cp_conv3x3_winograd24_group_f32(const cp_conv_desc* d, int n, const float* const* src, const float* const* u,
                                    const float* const* scale, const float* const* shift, const float* const* res,
                                    float* const* out, void* stream);

/* One KeypointHead branch (lib/models/heads/keypoint.py:14-37: conv3x3(C -> head_conv, bias) -> ReLU -> conv1x1(head_conv -> n, bias))
 * with n <= 34 outputs -- all six branches of the reference head -- as ONE launch: the 1x1 is applied to every channel tile of the
 * Winograd kernel while it is on the CU (n <= 2: in the epilogue registers; more: a second MFMA phase over the LDS-resident tile),
 * the [B,H,W,head_conv] intermediate is never written.  d / src / u / scale / shift: the 3x3 conv as for
 * cp_conv3x3_winograd_f32 (C = 64, act = CP_ACT_RELU); w2: [n2][ld2] (ld2 >= head_conv, % 4 == 0), b2: [n2]; out2: NCHW
 * [B,n2,H,W]; act2: CP_ACT_SIGMOID for hm (lib/detectors/multi_pose.py:35-37), else CP_ACT_NONE.  Returns 1 for other shapes. */
int cp_head3x3_1x1_f32(const cp_conv_desc* d, const float* src, const float* u, const float* scale, const float* shift,
                       const float* w2, const float* b2, float* out2, int n2, int ld2, int act2, void* stream);

/* ---- fused DCNv2 forward -------------------------------------------------------------------------
 * Replaces dcn_v2_forward / dcn_v2_cuda_forward (DCNv2/src/dcn_v2.h:9-39, src/cuda/dcn_v2_cuda.cu:42-172,
 * src/cuda/dcn_v2_im2col_cuda.cu:25-54,125-195) plus the BN + ReLU of DeformConv (pose_dla_dcn.py:345-348).
 * x: NHWC [B,H,W,srcLd]; om: NHWC [B,Ho,Wo,omLd] with ch 2k = dy_k, 2k+1 = dx_k, 2*kh*kw + k = mask_k
 * (logits if omSigmoid, as produced by conv_offset_mask, dcn_v2.py:117-121; already-sigmoided otherwise);
 * w: [ldw][kh*kw*C]; deformable groups: `dg` below (the reference's models only use 1, pose_dla_dcn.py:343; the interface
 * implements any, dcn_v2_im2col_cuda.cu:153,162-164). */
typedef struct cp_dcn_desc {
    int B, H, W, C, srcLd;
    int Ho, Wo;
    int kh, kw, sy, sx, py, px, dily, dilx;
    int K, ldw, Cout;
    int omLd, omSigmoid;
    int outLd, outNCHW, act;
    int tile;
    int ksplit;     /* 0 / 1: none.  S > 1: split-K over the taps for small-M layers: `out` is a workspace [S][B*Ho*Wo][ldw] that receives
                     * the raw partial sums (scale = ones, shift = zeros, act = CP_ACT_NONE, NHWC, outLd = Cout = ldw);
                     * cp_splitk_reduce_f32 sums the S slices in a fixed order (deterministic) and applies scale / shift / act */
    int dg;         /* 0 / 1: one deformable group.  G > 1: input channel c samples with the offsets / mask of group g = c / (C / G)
                     * ((C / G) % 16 == 0): om channel 2 * (g * kh*kw + k) = dy, + 1 = dx, 2 * G * kh*kw + g * kh*kw + k = mask;
                     * omLd >= 3 * G * kh*kw */
} cp_dcn_desc;
int cp_dcn_v2_f32(const cp_dcn_desc* d, const float* x, const float* om, const float* w, const float* scale,
                  const float* shift, float* out, void* stream);
/* Kernel-side constants of a DCNv2 layer from the reference's parameters, one launch: w [Co][C][kh][kw] and bias [Co]
 * (nn.Parameter layout, DCNv2/dcn_v2.py:99-103) -> wp [ldw][kh*kw*Cp] (k = (tap*dg + g)*(Cp/dg) + c, zero padding), scale [ldw] = 1,
 * shift [ldw] = bias -- the `w`, `scale`, `shift` of cp_dcn_v2_f32.  The drop-in dcn_v2_forward (DCNv2/src/dcn_v2.h:9-23) calls it
 * on every forward: no packed-weight cache to go stale. */
int cp_dcn_pack_weights_f32(const float* w, const float* bias, int Co, int C, int kh, int kw, int dg, int Cp, int ldw, float* wp,
                            float* scale, float* shift, void* stream);
/* sizeof the two descriptor structs as THIS library was compiled: an FFI binder (ctypes, cgo, JNI) asserts its own layout against
 * them, and the plan runtime rejects plan files whose descriptor blobs have another size */
int cp_sizeof_conv_desc(void);
int cp_sizeof_dcn_desc(void);

/* second half of a split-K DCNv2 launch: out[m][n] = act((sum_s ws[s][m][n]) * scale[n] + shift[n]), n < Cout; NHWC out */
int cp_splitk_reduce_f32(const float* ws, int splits, int M, int ldw, const float* scale, const float* shift, int act, float* out,
                         int outLd, int Cout, void* stream);

/* ---- 7x7 / pad 3 stem on the NCHW 3-channel network input ----------------------------------------
 * Replaces base_layer Conv2d(3,16,k7,s1,p3)+BN+ReLU (pose_dla_dcn.py:228-232) and conv1 Conv2d(3,64,k7,s2,p3)
 * +BN+ReLU (msra_resnet.py:118-121).  x: NCHW [B,3,H,W]; w: [Cout][176] with k = ((c*7+ky)*8 + kx) (kx padded
 * to 8, zeros); out: NHWC [B,Ho,Wo,outLd].  (Cout, stride) in {16,64} x {1,2}. */
int cp_stem7x7_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int B, int H, int W,
                   int Cout, int stride, int outLd, int relu, void* stream);

/* ---- bandwidth-bound NHWC helpers --------------------------------------------------------------- */
/* nn.MaxPool2d (pose_dla_dcn.py:197-198 k2 s2; msra_resnet.py:123 k3 s2 p1) */
int cp_maxpool2d_nhwc_f32(const float* in, int inLd, float* out, int outLd, int B, int H, int W, int C, int k, int s, int p,
                          void* stream);
/* IDAUp: depthwise ConvTranspose2d(k=2f, s=f, p=f/2, groups=C) + add (pose_dla_dcn.py:360-377); w: [k*k][C] */
int cp_dw_deconv_add_nhwc_f32(const float* in, int inLd, const float* w, const float* add, int addLd, float* out, int outLd,
                              int B, int H, int W, int C, int f, void* stream);
/* HRNet fuse: out = relu?( sum_i nearest_upsample(src_i, 2^shift_i) ) (pose_higher_hrnet.py:217-235) */
int cp_sum_up_nhwc_f32(int n, const float* const* src, const int* ld, const int* shift, float* out, int outLd, int B, int H,
                       int W, int C, int relu, void* stream);
/* Up to four INDEPENDENT sums of that kind in ONE launch (the y_i = relu(sum_j fuse_ij(x_j)) of every output branch of an HRNet module,
 * pose_higher_hrnet.py:224-235); bit-identical to the single launches.  src: 4 pointers per member (NULL beyond its source count);
 * meta: 14 ints per member = nsrc, ld[4], shift[4], outLd, B, H, W, C; out: one NHWC output per member (they must not alias). */
int cp_sum_up_group_nhwc_f32(int n, const float* const* src, const int* meta, float* const* out, int relu, void* stream);
/* depthwise k x k conv + folded BN + activation (groups == channels): MobileNetV3 Block.conv2 (mobilenetv3.py:119-121, k 3 / 5,
 * stride 1 / 2) and ShuffleNetV2 banch1 / banch2 (shufflenetv2_dcn.py:67-88); w: [k*k][C], scale / shift: [C] */
int cp_dwconv2d_nhwc_f32(const float* in, int inLd, const float* w, const float* scale, const float* shift, float* out, int outLd,
                         int B, int H, int W, int C, int k, int s, int p, int act, void* stream);
/* SeModule (mobilenetv3.py:99-113): nn.AdaptiveAvgPool2d(1) of in [B,HW,C] -> out [B,C]; then out = x * se[b,c] (+ add:
 * the block's shortcut, mobilenetv3.py:141-143) */
int cp_global_avgpool_nhwc_f32(const float* in, int inLd, float* out, int outLd, int B, int HW, int C, void* stream);
int cp_scale_add_nhwc_f32(const float* x, int xLd, const float* se, int seLd, const float* add, int addLd, float* out, int outLd,
                          int B, int H, int W, int C, void* stream);
/* The tail of the DeepSort re-id net (demo/tracking/model.py:88-92: AvgPool2d over the whole map, x.div(x.norm(p=2, dim=1))):
 * in [B,HW,C] (pixel stride inLd >= C) -> out [B,C] (row stride outLd >= C) = m / ||m||_2 with m the mean over HW.  No epsilon, as
 * there: an all-zero map gives NaN.  One block per image, fixed summation order; B <= 65535. */
int cp_pool_l2norm_nhwc_f32(const float* in, int inLd, float* out, int outLd, int B, int HW, int C, void* stream);
/* channel_shuffle(torch.cat((x1, x2), 1), 2) of ShuffleNetV2 (shufflenetv2_dcn.py:28-42,94-104); x1, x2: h channels each;
 * out: two halves of hp (>= h, multiple of 16) physical channels, logical channel c -> c (c < h) or hp + c - h; pads = 0 */
int cp_shuffle_concat_nhwc_f32(const float* x1, int ld1, const float* x2, int ld2, float* out, int outLd, long long npix, int h, int hp,
                               void* stream);
int cp_nchw_to_nhwc_f32(const float* in, float* out, int B, int C, int H, int W, int outLd, int cOff, void* stream);
int cp_nhwc_to_nchw_f32(const float* in, int inLd, int cOff, float* out, int B, int C, int H, int W, void* stream);
int cp_fill_f32(float* p, float v, long long n, void* stream);
/* flip-test merge (multi_pose.py:45-53; models/utils.py:27-47): in [2,C,H,W] NCHW -> out [1,C,H,W];
 * mode 0 = W-flip average (hm, wh); 1 = + left/right joint swap (hm_hp); 2 = swap on (x,y) pairs + negate x (hps).
 * perm: device int[J] joint permutation (NULL for mode 0). */
int cp_flip_merge_f32(const float* in, float* out, int C, int H, int W, int mode, const int* perm, void* stream);
/* the same merge for N image / mirrored-twin pairs and up to four maps in ONE launch: in[k] NCHW [2N,C_k,H,W] with image n at batch
 * 2n and its twin at 2n + 1 -> out[k] [N,C_k,H,W]; meta: [n][2] = C_k, mode_k with modes 0..2 as above and 3 = copy of the image's
 * own plane (reg, hp_offset: multi_pose.py:52-53).  Bit-identical to cp_flip_merge_f32 per pair.  perm: device int[J] (modes 1, 2:
 * C_k = J resp. 2J).  W % 4 == 0 with 16-B aligned maps takes a float4 path, anything else a scalar one. */
int cp_flip_merge_pairs_f32(int n, const float* const* in, float* const* out, const int* meta, int N, int H, int W, int J,
                            const int* perm, void* stream);

/* ---- device pre-/post-processing ---------------------------------------------------
 * The 8-bit pixel arithmetic is OpenCV's (opencv-python, unpinned, requirements.txt): resize.cpp / imgwarp.cpp fixed-point
 * bilinear paths, restated in oracle/prepost_np.py; parity against cv2 itself is unpinned (cv2 is not installable here).
 * cp_resize_u8: cv2.resize(image, (NW, NH)) with the default INTER_LINEAR (base_detector.py:47); DEVICE uint8 [H,W,3] ->
 *   DEVICE uint8 [NH,NW,3].
 * cp_preprocess_u8_f32: cv2.warpAffine(INTER_LINEAR, border 0) + (x/255 - mean)/std + HWC->CHW of
 *   lib/detectors/base_detector.py:48-56.  img: DEVICE uint8 [H,W,3]; M: HOST double[6], the 2x3 matrix given to
 *   warpAffine (source -> destination, `trans_input`); mean/std_: HOST float[3];
 *   out: DEVICE float32 NCHW [1 or 2,3,OH,OW]; flip != 0 also writes the mirrored twin as batch entry 1 (:57-58).
 * cp_transform_dets_f32: lib/utils/post_process.py:8-19 + lib/utils/image.py:19-24 on the device: the 2 box corners
 *   and J keypoints of dets[B,K,5+3J] through the per-image 2x3 double matrix trans[B][6], then / scale. */
int cp_resize_u8(const unsigned char* src, int H, int W, unsigned char* dst, int NH, int NW, void* stream);
int cp_preprocess_u8_f32(const unsigned char* img, int H, int W, const double* M, float* out, int OH, int OW, const float* mean,
                         const float* std_, int flip, void* stream);
int cp_transform_dets_f32(const float* dets, float* out, const double* trans, int B, int K, int J, float scale, void* stream);

/* ---- heat-map decode -------------------------------------------------------------------------
 * Replaces multi_pose_decode(heat, wh, kps, reg, hm_hp, hp_offset, K)
 *   lib/models/decode.py:235-308 (with _nms :10-16, _topk :99-115, _topk_channel :87-96,
 *   _transpose_and_gather_feat lib/models/utils.py:11-25), called from
 *   lib/detectors/multi_pose.py:55.
 * heat[B,cat,H,W], hm_hp[B,J,H,W] are post-sigmoid NCHW float32; wh[B,2,H,W]; kps[B,2J,H,W];
 * reg / hp_offset [B,2,H,W] or NULL (then +0.5, decode.py:253-255,278-280).  hm_hp is mandatory
 * (the reference raises NameError without it).  dets[B,K,5+3J] float32 =
 * [x1,y1,x2,y2, score, (x,y)*J, joint_score*J] in feature-map pixels.
 * ws_scores[B,1+J,K] float32 / ws_inds[B,1+J,K] int32 are caller-owned scratch that also
 * returns the top-K peaks: plane 0 = person centres, plane 1+j = joint j candidates
 * (flat index y*W+x; order = value desc, index asc).
 * Limits: K <= 256 (the reference's TEST.TOPK is 100), K <= H*W.  Any map size: planes up to 32768 keys are
 * LDS-resident in one piece, larger ones (FIX_RES = false inputs, TEST_SCALES > 1) stream through LDS in chunks. */
int cp_decode_workspace_bytes(int B, int J, int K, size_t* scores_bytes, size_t* inds_bytes);
int cp_multi_pose_decode_f32(const float* heat, const float* wh, const float* kps, const float* reg,
                             const float* hm_hp, const float* hp_offset, int B, int cat, int J, int H,
                             int W, int K, float* dets, float* ws_scores, int* ws_inds, void* stream);
/* The same decode as two launches (cp_multi_pose_decode_f32 = both, back to back), for schedules that want them as two graph
 * nodes: cp_decode_topk_f32 = _nms + _topk + _topk_channel (decode.py:10-16,87-115) over hm / hm_hp -> ws_scores / ws_inds; it needs
 * only those two heads, so a two-stream schedule runs it beside the remaining head convolutions.  cp_decode_assign_f32 = the gathers
 * and the keypoint-to-person assignment (decode.py:240-308) -> dets. */
int cp_decode_topk_f32(const float* heat, const float* hm_hp, int B, int cat, int J, int H, int W, int K, float* ws_scores,
                       int* ws_inds, void* stream);
int cp_decode_assign_f32(const float* wh, const float* kps, const float* reg, const float* hp_offset, const float* ws_scores,
                         const int* ws_inds, int B, int J, int H, int W, int K, float* dets, void* stream);

/* ---- detections-only heads: wh / hps / reg at the centre peaks, hp_offset at the joint peaks -------------------------------
 * The four regression branches of the KeypointHead (keypoint.py:14-37: 3x3 conv C -> hc + bias + ReLU -> 1x1 conv hc -> n + bias)
 * evaluated ONLY at the pixels multi_pose_decode reads of them (decode.py:240-307), between cp_decode_topk_f32 and
 * cp_decode_assign_f32.  feat: the head input, NHWC [B,H,W,featLd] with C physical channels (C % 16 == 0, 16-B aligned rows);
 * ws_inds: cp_decode_topk_f32's [B,1+J,K] (row 0: centres, taken % (H*W); rows 1..J: joints).
 * w1: per branch (wh, hps, reg, hp_offset) [9C/8][2][hc][4], element (kb, h, n, s) = 3x3 weight of hidden channel n at
 * k = 8kb + 4h + s, k = tap * C + c (tap = ky * 3 + kx); b1: [4][hc]; w2: [6+2J][hc] = the 1x1 rows of wh (2), hps (2J), reg (2),
 * hp_offset (2); b2: [6+2J].  out: the four NCHW maps [B,n,H,W] back to back in that order (B*H*W*(6+2J) floats).  Writes every
 * channel of wh / hps / reg at every centre index and both hp_offset channels at every joint index, nothing else; a pixel's
 * values depend only on its 3x3 patch (duplicates are written with identical bits).  C <= 512; hc a multiple of 32 up to 256 or a multiple of 64 up to 512 (a block of
 * 2 hc resp. hc threads, 512 at most: hc = 288, 352, 416 and 480 are refused with rc 1).
 * Size limits (32-bit plane and row indices; larger is refused with rc 1): H*W < 2^31, B*H < 2^31 (pairs: 2*N*H), B*(1+J)*K < 2^31,
 * B*H*W*(6+2J) < 2^40. */
int cp_head_points_f32(const float* feat, int featLd, const int* ws_inds, const float* w1, const float* b1, const float* w2,
                       const float* b2, float* out, int B, int H, int W, int C, int J, int K, int hc, void* stream);
/* The same four branches under the flip test (multi_pose.py:45-53), at the peaks of the N MERGED heat maps.  feat: the head input of
 * the 2N images, pairs interleaved (image n at batch 2n, its mirrored twin at 2n + 1); ws_inds: cp_decode_topk_f32's [N,1+J,K] on
 * the merged hm / hm_hp; perm: the DEVICE joint permutation int[J] of cp_flip_merge_pairs_f32; w1 / b1 / w2 / b2: exactly as above.
 * out: the four MERGED maps [N,n,H,W] back to back (N*H*W*(6+2J) floats): wh and hps at a centre peak (y, x) are
 * (image(y, x) + sign * twin'(y, W-1-x)) / 2 with cp_flip_merge_pairs_f32's channel swap and sign (modes 0 and 2), each side bit for
 * bit what cp_head_points_f32 writes for that pixel of that image; reg and hp_offset are the image's own values (mode 3).  Same
 * write footprint and the same limits as cp_head_points_f32; one launch. */
int cp_head_points_pairs_f32(const float* feat, int featLd, const int* ws_inds, const int* perm, const float* w1, const float* b1,
                             const float* w2, const float* b2, float* out, int N, int H, int W, int C, int J, int K, int hc,
                             void* stream);

/* ---- plan handle: a whole network behind three calls -----------------------------
 * Replaces BackBoneWithHead.forward (lib/models/model.py:57-59: head_model(backbone_model(x))) for one compiled
 * (arch, B, H, W) and, with cp_plan_process, MultiPoseDetector.process (lib/detectors/multi_pose.py:29-60; the flip test
 * through a plan compiled with it, see cp_plan_flip_test) -- no Python involved.  A plan file / blob (layout: centerpose_amd/plan.py; written by Engine.save_plan) holds
 * the packed, BN-folded, Winograd-transformed constants and the schedule of the launches above.
 * cp_plan_load / cp_plan_create are the ONLY entry points of this library that allocate device memory (activation
 * buffers, constants; owned by the handle, released by cp_plan_destroy) and they synchronise the device once.
 * use_graph != 0: the first cp_plan_forward runs the schedule eagerly, captures it into a hipGraph, later calls replay it.
 * cp_plan_forward: images = DEVICE float32 NCHW [B,3,H,W] (mean/std-normalised, base_detector.py:53-58) or NULL when the
 *   caller wrote cp_plan_input() itself; enqueues on `stream`, no host synchronisation after the first call.
 * cp_plan_output: device pointer + NCHW shape of head i of [hm, wh, hps, reg, hm_hp, hp_offset] (keypoint.py:40-42);
 *   hm and hm_hp are already sigmoided (multi_pose.py:35-37 fused into the head epilogue).
 * cp_plan_process: forward + cp_multi_pose_decode_f32 -> dets DEVICE float32 [B,K,5+3J]. */
typedef struct cp_plan cp_plan;
/* FNV-1a (32 bit) of a host buffer: the checksum a CPPLAN04 file carries over everything behind its 48-byte header */
unsigned int cp_fnv1a32(const void* data, size_t bytes);
int cp_plan_load(const char* path, int use_graph, cp_plan** out);
int cp_plan_create(const void* blob, size_t bytes, int use_graph, cp_plan** out);
int cp_plan_info(const cp_plan* plan, int* B, int* H, int* W, int* n_outputs, int* n_launches);
float* cp_plan_input(const cp_plan* plan);
int cp_plan_output(const cp_plan* plan, int i, float** dev_ptr, int shape[4]);
int cp_plan_forward(cp_plan* plan, const float* images, void* stream);
int cp_plan_process(cp_plan* plan, const float* images, int K, float* dets, void* stream);
int cp_plan_destroy(cp_plan* plan);
/* 1 when the plan was compiled detections-only (Engine(..., decode_k=K, dets_only=True): it holds a cp_head_points_f32 launch; or
 * Engine(..., decode_k=K, flip_dets_only=True): a cp_head_points_pairs_f32 launch, and cp_plan_flip_test says 1 as well, the four
 * sparse outputs then being the [N] MERGED maps), else 0 (-1: NULL plan).  Such a plan still has six outputs, but outputs 1, 2, 3 and 5 (wh, hps, reg, hp_offset) are valid only at
 * the peaks the plan's own decode found; cp_plan_process / cp_pipeline_process need K = the plan's decode_k. */
int cp_plan_dets_only(const cp_plan* plan);
/* 1 when the plan was compiled for the flip test (Engine(..., decode_k=K, flip_test=True): it holds a cp_flip_merge_pairs_f32
 * launch), else 0 (-1: NULL plan).  Such a plan takes N image / mirrored-twin pairs as its batch B = 2N (image n at 2n, twin at
 * 2n + 1); its six outputs are the un-merged [2N] maps, and cp_plan_process / cp_pipeline_process write dets [N,K,5+3J] and need
 * K = the plan's decode_k. */
int cp_plan_flip_test(const cp_plan* plan);

/* ---- steps in flight (round 6): the C-ABI form of MultiPoseDetector.process_stream / engine.EnginePipeline ----------------------
 * Replaces nothing in the reference (it runs one image at a time, synchronously: lib/detectors/base_detector.py:79-140,
 * multi_pose.py:29-60); it is how the timed arrangement of bench.py is reached without Python.
 * cp_plan_clone: another INSTANCE of a loaded plan -- own activation buffers / static input / outputs / detections, the same
 *   constants (shared; freed with the last of the plan and its clones).  Destroy clones with cp_plan_destroy like any plan.
 * cp_pipeline_create: `depth` (1..8) instances of ONE plan (the plan and its clones, compiled with the decode inside the schedule:
 *   Engine(decode_k = K)) -> a handle that captures all their launch lists into ONE hipGraph on first use (both capture streams carry
 *   launches of several instances).  Does not take ownership of the plans; destroy the pipeline before its plans.
 * cp_pipeline_process: one replay = one step of EVERY instance.  images[k]: DEVICE float32 NCHW [B,3,H,W] (NULL = the caller filled
 *   cp_plan_input(plans[k]) itself); dets[k]: DEVICE float32 [B,K,5+3J] out ([B/2,K,5+3J] for a flip-test plan); per instance
 *   bit-identical to cp_plan_process.
 *   Enqueues on `stream`; the results of all instances are complete when the stream reaches the end of this call's work
 *   (throughput up, a batch's latency ~ depth x: INTEGRATION.md 3c). */
typedef struct cp_pipeline cp_pipeline;
int cp_plan_clone(const cp_plan* plan, cp_plan** out);
int cp_pipeline_create(cp_plan* const* plans, int depth, cp_pipeline** out);
int cp_pipeline_process(cp_pipeline* pipe, const float* const* images, int K, float* const* dets, void* stream);
int cp_pipeline_destroy(cp_pipeline* pipe);
/* HOST only, no plan handle and no device (plan tooling): the cross-stream event waits the plan runtime issues when it captures a
 * schedule on its two streams -- the same code path cp_plan_forward / cp_pipeline_process go through.  Op i runs on stream
 * streams[i] (0 main / 1 side), names nptr[i] pointers whose activation-buffer ids are listed flat, op after op, in bufids (-1:
 * constant / NULL; the ops of several plan instances: ids offset per instance) and writes the one at out_index[i] (plan.py: `ref`
 * ids, `out_index`, `stream` of every op); nbuf: number of buffers.  An op follows the last writer of every buffer it names and the
 * readers of the buffer it writes; of those on the other stream it waits for the youngest, unless its stream already waited for
 * that op or a younger one.  Writes up to `cap` (op, awaited op) pairs to HOST pairs[2 * cap] and returns how many there are
 * (possibly more than cap), -1 for a bad argument. */
int cp_schedule_waits(int n_ops, const int* streams, const int* nptr, const int* bufids, const int* out_index, int nbuf, int* pairs,
                      int cap);
/* stream-ordered device-to-device copy (for callers that keep a plan's outputs beyond the next forward) */
int cp_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* ---- the stages around the network for N images at once (MultiPoseDetector.run_batch) ---------------------------------------------
 * cp_pre_desc: one source image of a batched pre-process.  src_off: byte offset of its uint8 [H,W,3] pixels in ONE staging buffer;
 *   (NH,NW): the size cv2.resize brings it to (base_detector.py:47), mid_off: byte offset of that resized image in a scratch buffer,
 *   or < 0 when (NH,NW) == (H,W) (no resize); mi: the INVERTED 2x3 warp matrix (destination pixel -> resized-image coordinates),
 *   what cp_invert_warp makes of the matrix given to warpAffine -- the double operations of cp_preprocess_u8_f32; slot: the image's
 *   index in the output batch (its mirrored twin goes to slot + 1).
 * cp_preprocess_batch_u8_f32: cp_resize_u8 + cp_preprocess_u8_f32 for N images of different sizes and one network input size OH x OW:
 *   one resize launch (when any image has mid_off >= 0) and one warp launch, bit-identical to the per-image calls.  staging / scratch:
 *   DEVICE uint8 buffers of the given sizes; table: DEVICE cp_pre_desc[N], table_host: the same N descriptors on the HOST (every
 *   offset, size and slot is checked against the buffer sizes and out_batch before anything is launched); out: DEVICE float32
 *   [out_batch,3,OH,OW]; flip != 0 writes the twins.  OW % 4 == 0 with a 16-B aligned `out` takes a float4 store path.
 * cp_post_merge_batch_f32: for S <= 4 scales DEVICE dets[s] [N,K,56] -> out [N,S*K,56] (scale-major per image, as merge_outputs
 *   concatenates) and n_keep [N] (DEVICE int).  trans: DEVICE double [S][N][6], the feature-map -> image affine per (scale, image),
 *   with scales HOST float[S]: cp_transform_dets_f32's arithmetic; NULL: the rows are copied as they are.  nms != 0: soft_nms_39 per
 *   image on the device, one workgroup per image with its rows in LDS, cp_soft_nms_39's quirks kept (columns 0..38 move, 39..55 stay;
 *   copy of 0..4 and swap of 5..38 on a discard; all S*K rows are written, the kept ones first).  Bit-equal to cp_soft_nms_39 except
 *   that the Gaussian weight of method 2 uses the device's double exp (a decayed score may differ in its last float bit per decay).
 *   At most cp_post_merge_max_rows() = 512 rows per image with nms; more is an argument error.  Without nms n_keep[n] = S*K. */
typedef struct cp_pre_desc {
    long long src_off, mid_off;
    int H, W, NH, NW;
    double mi[6];
    int slot, pad;
} cp_pre_desc;
int cp_sizeof_pre_desc(void);
int cp_invert_warp(const double* M, double* Mi);
int cp_preprocess_batch_u8_f32(const unsigned char* staging, size_t staging_bytes, unsigned char* scratch, size_t scratch_bytes,
                               const void* table, const void* table_host, int N, float* out, int out_batch, int OH, int OW,
                               const float* mean, const float* std_, int flip, void* stream);
int cp_post_merge_max_rows(void);
int cp_post_merge_batch_f32(int S, const float* const* dets, const double* trans, const float* scales, int N, int K, float* out,
                            int* n_keep, int nms, float sigma, float Nt, float threshold, int method, void* stream);

/* ---- the batched pre-process from frames that are already on the device (run_batch / pre_process of CUDA tensors) -----------------
 * cp_frame_desc: one source frame, read IN PLACE.  Channel k (k = 0, 1, 2: the order the network and mean / std_ expect, cv2's B, G, R)
 *   of pixel (y, x) is the byte at base + y * row_stride + x * pix_stride + ch_off[k].  Packed BGR: (3W, 3, {0,1,2}); packed RGB:
 *   ch_off {2,1,0}; BGRA / RGBA: pix_stride 4 (byte 3 is never read); planar CHW: pix_stride 1, ch_off multiples of the plane stride;
 *   crops, padded rows and expanded views (a stride of 0) are the same rule.  H, W, NH, NW, mid_off, mi, slot: as in cp_pre_desc; the
 *   resized intermediate is packed [NH,NW,3] in network channel order.
 * cp_preprocess_frames_u8_f32: cp_preprocess_batch_u8_f32 with every source addressed through its descriptor instead of an offset into
 *   one staging buffer: one resize launch (when any frame has mid_off >= 0) and one warp launch, no repack and no copy of a frame,
 *   bit-identical to cp_preprocess_batch_u8_f32 on the equivalent packed BGR images.  table: DEVICE cp_frame_desc[N], table_host: the
 *   same descriptors on the HOST, checked before anything is launched: base non-null, sizes positive and below 2^29 pixels, strides and
 *   ch_off >= 0, the largest addressed offset below 2^62, mid_off / scratch / slot as for cp_preprocess_batch_u8_f32, N <= 65535.  The
 *   size of a frame's allocation is NOT known to the library: the caller vouches that every addressed byte is its own (a tensor view's
 *   shape, strides and data pointer do).  The frames are read when `stream` reaches the launches: they must have been produced in
 *   stream order before this call and stay allocated until that work has run.  cp_last_kernel(): preprocess_frames_kernel<vec4|scalar>. */
typedef struct cp_frame_desc {      /* 128 bytes */
    const unsigned char* base;      /* DEVICE address of pixel (0,0) */
    long long row_stride, pix_stride;   /* bytes */
    long long ch_off[3];            /* bytes from a pixel's address to network channel 0, 1, 2 */
    long long mid_off;              /* as cp_pre_desc: offset of the resized image in scratch, < 0: no resize */
    int H, W, NH, NW;
    double mi[6];                   /* inverted warp matrix (cp_invert_warp) */
    int slot, pad;
} cp_frame_desc;
int cp_sizeof_frame_desc(void);
int cp_preprocess_frames_u8_f32(const void* table, const void* table_host, int N, unsigned char* scratch, size_t scratch_bytes,
                                float* out, int out_batch, int OH, int OW, const float* mean, const float* std_, int flip, void* stream);

/* ---- the same from device frames in 4:2:0 YUV: NV12 (a hardware decoder's surface), NV21, I420 / YV12 -----------------------------
 * cp_yuv_frame_desc: one source frame of 8-bit planes, read IN PLACE.  Y(r, c) is the byte at y_base + r * y_row + c * y_pix, U(r, c)
 *   the byte at u_base + (r >> 1) * c_row + (c >> 1) * c_pix, V(r, c) the same expression from v_base: the chroma of a pixel is the
 *   nearest sample, one (U, V) pair per 2x2 block, no chroma interpolation.  NV12: v_base = u_base + 1, c_pix = 2; NV21: u_base =
 *   v_base + 1, c_pix = 2; I420 / YV12: two chroma planes, c_pix = 1.  Pitched rows, crops at even origins and expanded planes (a
 *   stride of 0) are the same rule; H or W may be odd, the chroma planes then hold (H + 1) / 2 x (W + 1) / 2 samples.  mid_off, H, W,
 *   NH, NW, mi, slot: as in cp_frame_desc; the resized intermediate is packed [NH,NW,3] BGR.
 * The conversion (csrc/yuv_arith.h) is integer-only.  coef = (CY, CVR, CVG, CUG, CUB, YOFF), HOST int[6]; in int32, arithmetic shifts:
 *       y = max(Y - YOFF, 0) * CY;  u = U - 128;  v = V - 128
 *       R = clamp((y + CVR * v + (1 << 19)) >> 20, 0, 255)
 *       G = clamp((y + CVG * v + CUG * u + (1 << 19)) >> 20, 0, 255)
 *       B = clamp((y + CUB * u + (1 << 19)) >> 20, 0, 255)
 *   limited-range BT.601: (1220542, 1673527, -852492, -409993, 2116026, 16) -- the constants, rounding term and shift of
 *   cv2.cvtColor(COLOR_YUV2BGR_NV12), restated, not pinned to a recording; limited-range BT.709: (1220542, 1880097, -558891, -223347,
 *   2214593, 16).  Any other matrix goes if it cannot overflow int32: CY > 0, 0 <= YOFF <= 255 and
 *   255 * CY + (1 << 19) + 128 * max(|CVR|, |CVG| + |CUG|, |CUB|) < 2^31; anything else is an argument error.
 * cp_preprocess_yuv_frames_u8_f32: cp_preprocess_frames_u8_f32 for such frames: one resize launch (when any frame has mid_off >= 0) and
 *   one warp launch, bit-identical to cp_preprocess_frames_u8_f32 on the packed [H,W,3] BGR image obtained by converting every pixel of
 *   the frame (per source pixel, before the resize and before the warp).  table: DEVICE cp_yuv_frame_desc[N], table_host: the same
 *   descriptors on the HOST, checked before anything is launched: the three bases non-null, sizes positive and below 2^29 pixels,
 *   strides >= 0, every plane's largest addressed offset below 2^62, mid_off / scratch / slot as for cp_preprocess_frames_u8_f32,
 *   N <= 65535, and coef as above.  The caller vouches for the planes' memory, stream order and lifetime exactly as for cp_frame_desc,
 *   per plane.  cp_last_kernel(): preprocess_yuv_frames_kernel<vec4|scalar>.
 * cp_yuv_to_bgr_host: HOST only -- the conversion of n (Y, U, V) triples to bgr[3 * n] by the same statements the kernels compile.
 * Format word: the descriptor's trailing `pad` says what the planes hold (csrc/yuv_source.h); 0 is everything above.
 *       bit 0  chroma not subsampled horizontally        bit 2  16-bit samples, little-endian; strides stay in BYTES
 *       bit 1  chroma not subsampled vertically           bit 3  no chroma planes (grey): U = V = mid-scale, u_base / v_base may be null
 *   U(r, c) is the sample at u_base + (r >> sy) * c_row + (c >> sx) * c_pix with (sx, sy) = (1, 1) for 4:2:0 (word 0), (1, 0) for 4:2:2
 *   (word 2; packed YUYV / UYVY is this with c_pix = 2 * y_pix), (0, 0) for 4:4:4 (word 3); P010 / P016 are word 4 with the NV12
 *   addresses in bytes; the bits are orthogonal (16-bit 4:4:4 is word 7).  Values above 15, bit 3 together with bit 0 or 1, and an odd
 *   base or stride of 16-bit samples are argument errors.  8-bit samples convert as above, grey with U = V = 128.  16-bit samples are
 *   used as stored, s in [0, 65535] (P010: ten bits in the MSBs; whatever the low six bits hold counts), in int64:
 *       yy = max(Y - 256 * YOFF, 0);  u = U - 32768;  v = V - 32768
 *       R = clamp((CY * yy + CVR * v + (1 << 27)) >> 28, 0, 255)       G: CVG * v + CUG * u       B: CUB * u
 *   so that a frame holding x << 8 converts to exactly the bytes the 8-bit rule gives for x.  Each sample is ONE 2-byte load; an
 *   interleaved pair is never assumed to be 4-byte aligned.  Full-range and BT.2020 rows of coef, the closed form round(k * 2^20):
 *   bt601-full (1048576, 1470104, -748826, -360853, 1858077, 0), bt709-full (1048576, 1651297, -490864, -196424, 1945738, 0),
 *   bt2020-limited (1220945, 1760217, -682019, -196426, 2245811, 16), bt2020-full (1048576, 1546230, -599107, -172546, 1972791, 0).
 *   A launch whose frames all have word 0 runs the kernels it always ran; with any other word in the table ALL its frames go through
 *   the general instantiations and cp_last_kernel() is preprocess_yuv_surfaces_kernel<vec4|scalar> (reid_crop_kernel<surfaces> for
 *   cp_reid_crop_yuv_frames_f32; the selection stays reid_select_kernel<yuv>).  The cp_draw_* entry points, device and host, refuse a
 *   non-zero word with an argument error that names `pad`: they write 8-bit 4:2:0 only.
 * cp_yuv16_to_bgr_host: HOST only -- cp_yuv_to_bgr_host for n triples of 16-bit container values. */
typedef struct cp_yuv_frame_desc {  /* 136 bytes */
    const unsigned char* y_base;    /* DEVICE address of Y(0,0) */
    long long y_row, y_pix;         /* bytes */
    const unsigned char* u_base;    /* DEVICE address of U(0,0) */
    const unsigned char* v_base;    /* DEVICE address of V(0,0) */
    long long c_row, c_pix;         /* bytes per chroma row / per chroma sample, both chroma planes */
    long long mid_off;              /* as cp_pre_desc: offset of the resized image in scratch, < 0: no resize */
    int H, W, NH, NW;
    double mi[6];                   /* inverted warp matrix (cp_invert_warp) */
    int slot, pad;                  /* pad: the format word, 0 = 8-bit 4:2:0 */
} cp_yuv_frame_desc;
int cp_sizeof_yuv_frame_desc(void);
int cp_preprocess_yuv_frames_u8_f32(const void* table, const void* table_host, int N, const int* coef, unsigned char* scratch,
                                    size_t scratch_bytes, float* out, int out_batch, int OH, int OW, const float* mean, const float* std_,
                                    int flip, void* stream);
int cp_yuv_to_bgr_host(const unsigned char* y, const unsigned char* u, const unsigned char* v, size_t n, const int* coef,
                       unsigned char* bgr);
int cp_yuv16_to_bgr_host(const unsigned short* y, const unsigned short* u, const unsigned short* v, size_t n, const int* coef,
                         unsigned char* bgr);

/* ---- draw the detections onto device frames, in place (draw_results / run_batch(draw=True)) ------------------------------------------
 * The box, the 18 limbs and the 17 joints of every row of rows[N,M,56] (box 0:4, score 4, joints 5:39, joint scores 39:56, image
 * coordinates) whose score is > vis_thresh, painted onto frame n = 0..N-1 with its own M rows.  Opaque: a frame is never read; bytes
 * that no primitive covers -- a fourth channel, row padding, everything outside H x W -- are not written.  The picture is this library's
 * own rule (csrc/draw_arith.h), integer-only after the first step:
 *   coordinates: a non-finite one (by the float's bits) kills its primitive; any other is clamped to [-16384, 16383] and truncated
 *     toward zero.  Primitives of a row in paint order, the index being the palette entry: 0 the box (exists iff its four coordinates
 *     are alive), 1..18 the limbs (0,1) (0,2) (1,3) (2,4) (3,5) (4,6) (5,6) (5,7) (7,9) (6,8) (8,10) (5,11) (6,12) (11,12) (11,13) (13,15)
 *     (12,14) (14,16) (both joint scores > 0, four coordinates alive), 19..35 the joints (score > 0, both coordinates alive).
 *   coverage of pixel p, k = R * R + R: joint at P: |p - P|^2 <= k.  Limb P -> Q: a = p - P, d = Q - P, L2 = d.d, t = a.d; L2 = 0 or
 *     t <= 0: a.a <= k; t >= L2: |p - Q|^2 <= k; otherwise (a x d)^2 <= k * L2.  Box of thickness T, corners sorted: inside the closed
 *     rectangle and x - x0 < T or x1 - x < T or y - y0 < T or y1 - y < T.
 *   order: rows ascending, primitives in paint order, the last one that covers a pixel gives its colour.
 * cp_draw_style: box_thickness 0..64 (0: no box), limb_radius -1 (no limbs) or 1..64, joint_radius -1 (no joints) or 0..64; palette[l]
 *   bytes 0..2: what primitive l stores -- for cp_frame_desc frames byte k goes to ch_off[k] (k = 0, 1, 2: B, G, R of a BGR or RGB
 *   frame described as for the pre-process), for cp_yuv_frame_desc frames they are (Y, U, V).  Byte 3 is not used.
 * cp_draw_rows_frames_u8 / cp_draw_rows_yuv_frames_u8: two launches on `stream` (draw_build_kernel: one wave per row builds the
 *   primitive records and the row's bounding box into scratch; draw_raster_kernel: one block per 16x16 pixel tile -- 32x32 for YUV,
 *   where a thread owns a 2x2 block -- and frame finds every pixel's last covering primitive and stores it).  table: DEVICE
 *   cp_frame_desc[N] / cp_yuv_frame_desc[N], table_host: the same descriptors on the HOST; only the addressing fields and H, W are
 *   read.  rows: DEVICE float32 [N,M,56].  style: HOST.  scratch: DEVICE, 16-byte aligned, at least cp_draw_scratch_bytes(N, M) bytes,
 *   contents undefined before and after.  YUV frames: luma per covered pixel; chroma sample (i, j) is written iff one of the luma
 *   pixels (2i..2i+1, 2j..2j+1) inside the frame is covered and takes the colour of the latest-painted winner among them.
 *   Checked before anything is launched (rc 1, cp_last_error): null pointers, 0 <= N <= 65535, 0 <= M <= 2^24 and N * M <= 2^28, a
 *   finite vis_thresh, the style ranges, the scratch size and alignment, and per frame: bases non-null, H and W in 1..16384, no negative
 *   stride or offset, a positive stride along every dimension with more than one index, distinct ch_off / distinct U and V bases,
 *   addressed offsets below 2^62.  N = 0 or M = 0 succeeds and launches nothing.  The caller vouches for the frames' memory, stream
 *   order and lifetime as for the pre-process, and ALSO that no two addressed bytes of one call coincide (within a frame or between
 *   frames): a frame is written here.  cp_last_kernel(): draw_raster_kernel<bgr|yuv>.
 * cp_draw_rows_frames_host / cp_draw_rows_yuv_frames_host: HOST only -- sequential painters over the same descriptors holding host
 *   addresses and host rows, built from the same statements; same checks.  What the device result is pinned to, byte for byte. */
typedef struct cp_draw_style {      /* 156 bytes */
    int box_thickness;
    int limb_radius;
    int joint_radius;
    unsigned char palette[36][4];
} cp_draw_style;
int cp_sizeof_draw_style(void);
size_t cp_draw_scratch_bytes(int N, int M);
int cp_draw_rows_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                           const void* style, void* scratch, size_t scratch_bytes, void* stream);
int cp_draw_rows_yuv_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                               const void* style, void* scratch, size_t scratch_bytes, void* stream);
int cp_draw_rows_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style);
int cp_draw_rows_yuv_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style);

/* ---- poses in identity colours: the same painters with one colour per tracked row (draw_results(row_ids=) / run_batch(draw="tracks"))
 * cp_draw_rows_ids_*: exactly the entry point of the same name without `_ids` -- same launches, same checks, same coverage and painter's
 *   order -- with two more arguments: row_ids DEVICE (HOST for the *_host forms) int [N,M] and id_palette HOST cp_draw_id_palette.  A
 *   row whose id is >= 0 stores colors[id % count] for all 36 of its primitives; a row with id < 0 keeps the style's palette.  For
 *   cp_yuv_frame_desc frames the colours are (Y, U, V).  Also checked: both non-null, count in 1..64.  cp_last_kernel():
 *   draw_raster_kernel<bgr,ids|yuv,ids>.  With every id < 0 the result equals the plain entry point's byte for byte. */
typedef struct cp_draw_id_palette {     /* 260 bytes */
    int count;
    unsigned char colors[64][4];
} cp_draw_id_palette;
int cp_draw_rows_ids_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                               const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                               void* stream);
int cp_draw_rows_ids_yuv_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                   const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                                   void* stream);
int cp_draw_rows_ids_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                 const int* row_ids, const void* id_palette);
int cp_draw_rows_ids_yuv_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                     const int* row_ids, const void* id_palette);

/* ---- score labels and translucent poses: draw_results with an overlay (DrawStyle(labels=..., limb_opacity=...)) -----------------------
 * What the reference's show_results adds to the boxes and skeletons above: '{prefix}{score:.1f}' on a filled bar on top of every box
 * (Debugger.add_coco_bbox) and limbs blended into the picture (Debugger.add_coco_hp).  The rule is csrc/draw_overlay_arith.h:
 *   primitives of a row in paint order: the 36 of cp_draw_style, then 36 the label bar and 37 the label text; paint index row * 38 + l.
 *   blend: primitive l has an opacity a in 1..256 -- opacity[0] the box, [1] the limbs, [2] the joints, bar and text always 256 -- and a
 *     covered channel byte p becomes (p * (256 - a) + c * a + 128) >> 8, once per covering primitive, in paint order (a = 256: c).  YUV
 *     frames: luma per covered pixel; chroma sample (i, j) once per primitive that covers at least one in-frame pixel of its 2x2 block,
 *     with that primitive's (U, V).  A frame is READ where a translucent primitive covers it and nothing opaque lies beneath.
 *   label: a live row has one iff label_scale s is in 1..8 and its four box coordinates are alive (box_thickness plays no part).  With
 *     (x0, y0) the box's sorted corner, n characters, tw = 6 s n - s, th = 7 s: the bar is the closed rectangle [x0, x0 + tw + 3] x
 *     [y0 - th - 5, y0 - 1] in the colour the row's box takes (palette[0] or the identity colour); the text follows the glyph rule of
 *     cp_draw_track_item with dx = x - (x0 + 2), dy = y - (y0 - th - 3), in text_color.  What leaves the frame is clipped.
 *   text: prefix[0 .. nprefix - 1] (glyph indices, nprefix 0..9), then the score to one decimal by an integer rule on the float's bits:
 *     with |score| = m 2^e exactly, t = min(round_half_even(10 m 2^e), 9999); ['-' if the sign bit is set] str(t / 10) '.' str(t % 10).
 *     +-inf gives 999.9; this is '%.1f' for |score| < 999.95.  cp_draw_score_label runs it on the HOST: glyphs[0..5] -> nchars, -1 for NaN.
 * cp_draw_overlay_frames_u8 / cp_draw_overlay_yuv_frames_u8: the arguments of cp_draw_rows_ids_*_u8 and `overlay`, a HOST cp_draw_overlay;
 *   row_ids and id_palette may both be null.  Two launches on `stream` (draw_overlay_build_kernel: draw_build_kernel, which also turns
 *   the score into the row's label record; draw_overlay_kernel: the tiles and pixel ownership of draw_raster_kernel, the topmost
 *   opaque cover from the back, then the translucent primitives above it forward).  scratch: cp_draw_overlay_scratch_bytes(N, M).
 *   Checked before anything is launched: all that cp_draw_rows_ids_* checks, a non-null overlay, opacities in 1..256, label_scale in
 *   0..8, nprefix in 0..9, every prefix glyph inside the font, row_ids and id_palette both null or both non-null.  With opacities 256
 *   and label_scale 0 the result equals cp_draw_rows_* / cp_draw_rows_ids_* byte for byte.  cp_last_kernel(): draw_overlay_kernel<bgr|yuv>.
 * cp_draw_overlay_frames_host / cp_draw_overlay_yuv_frames_host: HOST only -- the sequential painters, same statements, same checks.
 *   What the device result is pinned to, byte for byte. */
typedef struct cp_draw_overlay {        /* 36 bytes */
    int opacity[3];
    int label_scale;
    int nprefix;
    unsigned char prefix[12];
    unsigned char text_color[4];
} cp_draw_overlay;
int cp_sizeof_draw_overlay(void);
size_t cp_draw_overlay_scratch_bytes(int N, int M);
int cp_draw_score_label(float score, unsigned char* glyphs);
int cp_draw_overlay_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                              const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                              const void* overlay, void* stream);
int cp_draw_overlay_yuv_frames_u8(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                                  const void* style, void* scratch, size_t scratch_bytes, const int* row_ids, const void* id_palette,
                                  const void* overlay, void* stream);
int cp_draw_overlay_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                const int* row_ids, const void* id_palette, const void* overlay);
int cp_draw_overlay_yuv_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const void* style,
                                    const int* row_ids, const void* id_palette, const void* overlay);

/* ---- heat maps blended over device frames, in place: the debug views pred_hm / pred_hmhp (draw_heatmaps) ----------------------------------
 * What the reference's MultiPoseDetector.debug shows: the centre heat map or the 17 joint heat maps as a colour map (Debugger.gen_colormap /
 * gen_colormap_hp) blended over the picture (add_blend_img).  Every pixel of every frame is read and written.  The rule is
 * csrc/draw_heat_arith.h:
 *   colour map, per image and map cell: m_k = max over c < C of (v_c * palette[c][k]) for k in B, G, R -- one float32 multiply per term,
 *     from 0 and compared with '>', so a NaN never wins and negatives give 0 -- and cm_k = min(255, (int)m_k); with invert palette[c][k]
 *     is replaced by 255 - palette[c][k] and cm_k by 255 - cm_k.  Stored as uint8 [N, h, w, 4] in the scratch.
 *   position, per frame pixel (x, y), in double, with the frame -> map matrix T = the `mi` field of the frame's descriptor row (row major,
 *     finite): mx = T[0] x + T[1] y + T[2] left to right, clamped to [0, w - 1], X = (long long)(mx * 256.0 + 0.5), ix = X >> 8,
 *     fx = X & 255, ix1 = min(ix + 1, w - 1); my from T[3..5] and h alike.  Cell (i, j) sits AT map coordinate (i, j); outside the map
 *     the border repeats.
 *   sample, per component: t0 = a (256 - fx) + b fx on row iy, t1 on row iy1, f = (t0 (256 - fy) + t1 fy + 32768) >> 16.
 *   blend: p' = (p (256 - opacity) + f opacity + 128) >> 8 on the three colour bytes; a fourth channel and padding keep their bytes.
 *   YUV frames (8-bit 4:2:0): f = (B, G, R) goes to (Y, U, V) by the limited-range forward form `matrix` (0: BT.601 Y = ((66 R + 129 G +
 *     25 B + 128) >> 8) + 16, ...; 1: BT.709), what cp_bgr_to_yuv_host computes; luma per pixel, a chroma sample with the (U, V) of the
 *     component-wise rounded mean (sum + (n >> 1)) / n of the fore colours of its n in {1, 2, 4} in-frame pixels.
 * maps: DEVICE float32, element (n, c, i, j) at maps[n s0 + c s1 + i s2 + j s3], any non-negative element strides; never copied.
 * style: HOST; `channels` palette entries (C..32) of (B, G, R), for the YUV form too.  scratch: DEVICE, 16-byte aligned,
 *   cp_draw_heat_scratch_bytes(N, h, w) bytes (0 when any argument is 0).
 * Two launches on `stream`: draw_heat_colormap_kernel (a thread per cell), draw_heat_blend_kernel<bgr_packed|bgr|yuv> -- <bgr_packed> when
 *   every frame of the call has pix_stride 3 and channel offsets (0,1,2) or (2,1,0): four pixels per thread as three aligned dwords, the
 *   ragged ends of a row byte-wise; otherwise <bgr>, a pixel per thread byte-wise; bit-identical.  cp_last_kernel() names the one that ran.
 * Checked before anything is launched: N in 0..65535 (0 succeeds and launches nothing), C in 1..32, channels in C..32, opacity in 1..256,
 *   invert 0 / 1, matrix 0 / 1, h and w in 1..16384, N h w <= 2^30, non-negative strides, non-null pointers, the scratch, the frames as for
 *   cp_draw_rows_*, a finite T per frame.
 * cp_draw_heat_frames_host / cp_draw_heat_yuv_frames_host: HOST only -- sequential painters over HOST maps, same statements, same checks.
 *   What the device result is pinned to, byte for byte. */
typedef struct cp_draw_heat_style {     /* 140 bytes */
    int channels;
    int opacity;
    int invert;
    unsigned char palette[32][4];
} cp_draw_heat_style;
int cp_sizeof_draw_heat_style(void);
size_t cp_draw_heat_scratch_bytes(int N, int h, int w);
int cp_bgr_to_yuv_host(const unsigned char* bgr, long long n, int matrix, unsigned char* yuv);
int cp_draw_heat_frames_u8(const void* table, const void* table_host, int N, const float* maps, long long s0, long long s1, long long s2,
                           long long s3, int C, int h, int w, const void* style, void* scratch, size_t scratch_bytes, void* stream);
int cp_draw_heat_yuv_frames_u8(const void* table, const void* table_host, int N, const float* maps, long long s0, long long s1, long long s2,
                               long long s3, int C, int h, int w, const void* style, int matrix, void* scratch, size_t scratch_bytes,
                               void* stream);
int cp_draw_heat_frames_host(const void* table_host, int N, const float* maps, long long s0, long long s1, long long s2, long long s3, int C,
                             int h, int w, const void* style);
int cp_draw_heat_yuv_frames_host(const void* table_host, int N, const float* maps, long long s0, long long s1, long long s2, long long s3,
                                 int C, int h, int w, const void* style, int matrix);

/* ---- draw tracks onto device frames, in place: box, label bar, label (draw_tracks / run_batch(draw="tracks")) --------------------------
 * What the reference's draw_bboxes puts on the picture per track, by this library's own integer rule (csrc/draw_text_arith.h) and its
 * own 5 x 7 font.  Frame n paints items[n][0 .. counts[n] - 1] of items[N][Kmax].  With box thickness T (0..64), font scale s (0..8,
 * 0: no bar and no text), tw = 6 s nchars - s, th = 7 s, an item has three primitives in paint order (paint index item * 3 + primitive):
 *   0 the box : corners (x0, y0) <= (x1, y1); inside the closed rectangle and x - x0 < T or x1 - x < T or y - y0 < T or y1 - y < T
 *   1 the bar : the closed rectangle [x0, x0 + tw + 3] x [y0, y0 + th + 4]; absent when nchars = 0 or s = 0
 *   2 the text: dx = x - (x0 + 2), dy = y - (y0 + 2); 0 <= dx < tw, 0 <= dy < th, u = (dx mod 6s) / s < 5 and bit (4 - u) of row dy / s
 *               of glyph[dx / 6s] set (bit 4: the leftmost column); absent with the bar
 *   order: items ascending, primitives in paint order, the last one that covers a pixel gives its colour -- color for box and bar,
 *   text_color for the text.  Opaque; a frame is never read; uncovered bytes are not written; what leaves the frame is clipped.
 *   YUV frames: colours are (Y, U, V); luma per covered pixel, chroma sample (i, j) as for cp_draw_rows_yuv_frames_u8.
 * cp_draw_track_item: corners sorted and in [-16384, 16383]; glyph: indices into the font -- 0..9 the digits, 10..35 A..Z, 36 space,
 *   37 '#', 38 '-', 39 '.', 40 ':', 41 '_' -- of which the first nchars (0..16) are read.
 * cp_draw_glyph_rows: the font.  rows[r], r = 0..6 from the top: bit 4 is the leftmost of five columns.  Returns the glyph index, -1 for
 *   a character outside the set (lower case included: the caller folds it) or a null `rows`.
 * cp_draw_tracks_frames_u8 / cp_draw_tracks_yuv_frames_u8: ONE launch on `stream` (draw_tracks_kernel: one block per 16x16 pixel tile --
 *   32x32 for YUV -- and frame walks the frame's items from the back).  table / items / counts: DEVICE; table_host / items_host /
 *   counts_host: the same bytes on the HOST, where everything is checked before anything is launched (rc 1, cp_last_error): null
 *   pointers, 0 <= N <= 65535, Kmax >= 0, N * Kmax <= 2^24, T in 0..64, s in 0..8, 0 <= counts[n] <= Kmax, nchars in 0..16, every read
 *   glyph index inside the font, sorted corners in range, and per frame what cp_draw_rows_frames_u8 checks.  N = 0, Kmax = 0 or no
 *   items at all succeeds and launches nothing.  The caller's promises are those of cp_draw_rows_frames_u8.  cp_last_kernel():
 *   draw_tracks_kernel<bgr|yuv>.
 * cp_draw_tracks_frames_host / cp_draw_tracks_yuv_frames_host: HOST only -- sequential painters over descriptors holding host addresses,
 *   built from the same statements; same checks.  What the device result is pinned to, byte for byte. */
typedef struct cp_draw_track_item {     /* 44 bytes */
    int x0, y0, x1, y1;
    unsigned char color[4];
    unsigned char text_color[4];
    int nchars;
    unsigned char glyph[16];
} cp_draw_track_item;
int cp_sizeof_draw_track_item(void);
int cp_draw_glyph_rows(int ch, unsigned char* rows);
int cp_draw_tracks_frames_u8(const void* table, const void* table_host, int N, const void* items, const void* items_host, const int* counts,
                             const int* counts_host, int Kmax, int box_thickness, int font_scale, void* stream);
int cp_draw_tracks_yuv_frames_u8(const void* table, const void* table_host, int N, const void* items, const void* items_host,
                                 const int* counts, const int* counts_host, int Kmax, int box_thickness, int font_scale, void* stream);
int cp_draw_tracks_frames_host(const void* table_host, int N, const void* items, const int* counts, int Kmax, int box_thickness,
                               int font_scale);
int cp_draw_tracks_yuv_frames_host(const void* table_host, int N, const void* items, const int* counts, int Kmax, int box_thickness,
                                   int font_scale);

/* ---- re-id crops: detections cut out of device frames into the re-id plan's input (reid.ReidExtractor / run_batch(embed=)) -------------
 * What DeepSort._get_features + Extractor._preprocess do per box on the host (demo/tracking/deep_sort.py:66-86,
 * feature_extractor.py:15-39), for every row of rows[N,M,56] and its own frame n, in two launches.  The values are this library's own
 * statement of that pipeline (csrc/reid_arith.h), not pinned to a cv2 recording:
 *   box: row = [x1, y1, x2, y2, score, ...]; the coordinates are clamped to +-2^30 and truncated toward zero; w = x2 - x1, h = y2 - y1,
 *     X1 = max(x1, 0), Y1 = max(y1, 0), X2 = min(X1 + w, W - 1), Y2 = min(Y1 + h, H - 1); the crop is rows Y1..Y2-1, columns X1..X2-1.
 *     A row is selected iff score > vis_thresh (strict; NaN is not), no coordinate is NaN and the crop has pixels.
 *   slots: with q = cap / N the first q selected rows of frame n, in row order, take slots n * q + 0, 1, ...
 *   pixel (oy, ox) of a crop of cw x ch pixels: fx = (ox + 0.5) * (cw / 64) - 0.5 in double, sx = floor(fx), weight f = float(fx - sx);
 *     sx < 0: column 0 alone, sx >= cw - 1: column cw - 1 alone, else columns sx, sx + 1 with float weights (1 - f, f); rows alike with
 *     ch / 128.  The four 8-bit taps are blended horizontally, then vertically, in double, rounded to float; then, in float,
 *     (v * scale - mean[k]) / std_[k].  Output channel k reads the frame's channel k of (B, G, R), or 2 - k with rgb = 1.
 * cp_reid_norm (HOST): scale, mean[3], std_[3], rgb.  The reference's values: scale 1 (its / 255 is commented out), mean (0.485, 0.456,
 *   0.406), std (0.229, 0.224, 0.225), rgb 0.
 * cp_reid_select_rows: one wave per frame -> slots[cap] DEVICE int (n * M + m, or -1 for an unused slot) and counts[N] DEVICE int (the
 *   selected rows per frame, NOT capped at q: a caller sees overflow without a synchronisation here).  table: DEVICE cp_frame_desc[N]
 *   (yuv = 0) or cp_yuv_frame_desc[N] (yuv = 1), table_host: the same on the HOST; only H and W are read.  rows: DEVICE float32 [N,M,56].
 * cp_reid_crop_frames_f32 / cp_reid_crop_yuv_frames_f32: out DEVICE float32 [cap,3,128,64], every element written: slot s holds the
 *   crop of row slots[s], zeros where slots[s] is -1 (or out of range, or not a selected row).  One thread per output pixel, frames
 *   read in place through the descriptors (addressing fields, H, W), YUV frames converted per source pixel with nearest chroma as in
 *   cp_preprocess_yuv_frames_u8_f32 (coef: HOST int[6], same rule).
 *   Checked before anything is launched (rc 1, cp_last_error): null pointers, cap in 1..4096, 1 <= N <= cap, M >= 0, N * M <= 2^24, and
 *   per frame: bases non-null, H, W positive and below 2^29 pixels, no negative stride or offset, addressed offsets below 2^62.  The
 *   caller vouches for the frames' memory, stream order and lifetime as for the pre-process; frames are only read, so expanded and
 *   overlapping views are fine.  cp_last_kernel(): reid_select_kernel<bgr|yuv>, reid_crop_kernel<bgr|yuv>.
 * cp_reid_*_host: HOST only -- sequential twins over descriptors holding host addresses, host rows / slots / out, built from the same
 *   statements; same checks.  What the device results are pinned to, bit for bit. */
typedef struct cp_reid_norm {       /* 32 bytes */
    float scale;
    float mean[3];
    float std_[3];
    int rgb;
} cp_reid_norm;
int cp_sizeof_reid_norm(void);
int cp_reid_select_rows(const void* table, const void* table_host, int yuv, int N, const float* rows, int M, float vis_thresh, int cap,
                        int* slots, int* counts, void* stream);
int cp_reid_crop_frames_f32(const void* table, const void* table_host, int N, const float* rows, int M, float vis_thresh,
                            const int* slots, int cap, const void* norm, float* out, void* stream);
int cp_reid_crop_yuv_frames_f32(const void* table, const void* table_host, int N, const int* coef, const float* rows, int M,
                                float vis_thresh, const int* slots, int cap, const void* norm, float* out, void* stream);
int cp_reid_select_rows_host(const void* table_host, int yuv, int N, const float* rows, int M, float vis_thresh, int cap, int* slots,
                             int* counts);
int cp_reid_crop_frames_host(const void* table_host, int N, const float* rows, int M, float vis_thresh, const int* slots, int cap,
                             const void* norm, float* out);
int cp_reid_crop_yuv_frames_host(const void* table_host, int N, const int* coef, const float* rows, int M, float vis_thresh,
                                 const int* slots, int cap, const void* norm, float* out);

/* ---- track association: the DeepSort appearance gallery and its cost matrix on the device (track.DeepSortTracker) ----------------------
 * What NearestNeighborDistanceMetric keeps and evaluates on the host (demo/tracking/sort/nn_matching.py:99-177): per track the last
 * `budget` feature vectors and, per frame, the smallest cosine distance of every detection to them.  S independent streams, Tcap track
 * slots per stream, q detection slots per stream; the state belongs to the caller and is passed as pointers:
 *   gallery DEVICE float32 [S * Tcap, budget, 512]: a ring of the last `budget` features per track slot, stored as given (not normalised);
 *   ginv    DEVICE float32 [S * Tcap, budget]: 1 / |row| of every ring row.
 * cp_track_cost_f32: one launch.  glen: DEVICE int [S * Tcap], the valid ring rows per slot (capped at budget; 0 = skip this slot);
 *   features DEVICE float32 [>= S * q, 512] and slots DEVICE int [>= S * q] as cp_reid_select_rows / the re-id plan leave them (slot
 *   s * q + d belongs to stream s; slots holds n * M + m or -1); rows DEVICE float32 [S, M, 56].  out: DEVICE float32, cost[S, Tcap, q]
 *   followed by det[S, q, 5]:
 *     cost[s, t, d] = min over g < glen[s, t] of 1 - <G[s, t, g], F[s * q + d]> * ginv[s, t, g] * (1 / |F[s * q + d]|), float32 products on
 *       the exact-f32 matrix cores; +inf where glen is 0 or the detection slot is unused (slots < 0 or >= S * M).  Ring rows >= glen are
 *       not read.  A NaN distance (a zero vector) does not take part in the min.
 *     det[s, d] = the first five floats (x1, y1, x2, y2, score) of row slots[s * q + d]; zeros for an unused slot.
 * cp_track_append_f32: one launch, one block per entry of table DEVICE int [n, 3] = (feature slot, track slot, ring position), the slots
 *   counted over all streams: the feature is copied into ring row (track slot, position) bit for bit and ginv gets 1.0f / sqrtf(float(sum
 *   of squares)), the sum taken in double in one fixed order (csrc/track_host.h) so that the device and the host twin write the same bits.
 *   An entry with a negative index or a position >= budget writes nothing.  The caller vouches that the indices lie inside its buffers and
 *   that no two entries name the same ring row; ordered after the cost launch by the stream.  n = 0 succeeds and launches nothing.
 *   Checked before anything is launched (rc 1, cp_last_error): budget in 1..128, Tcap in 1..1024, q >= 1, S in 1..65535, M >= 0, S * Tcap *
 *   budget ring rows <= 2^31 - 1 (rows are counted in int; every float offset is size_t), S * q and S * M <= 2^24, n in 0..2^24, null
 *   pointers, a gallery or feature pointer that is not 16-byte aligned.  cp_last_kernel(): track_cost_kernel, track_append_kernel.
 * cp_track_cost_host / cp_track_append_host: HOST only -- sequential twins over host arrays, same checks.  The append twin is what the
 *   kernel is pinned to bit for bit; the cost twin sums in float in k order and agrees with the kernel to rounding.
 * cp_linear_assignment_host: HOST only -- rectangular minimum-cost assignment of cost[rows, cols] (float64, row stride ld, finite) by
 *   shortest augmenting paths: min(rows, cols) pairs, row_to_col[r] = the column of row r or -1.  At most 4096 x 4096. */
int cp_track_cost_f32(const float* gallery, const float* ginv, const int* glen, const float* features, const int* slots, const float* rows,
                      int M, int S, int Tcap, int budget, int q, float* out, void* stream);
int cp_track_append_f32(float* gallery, float* ginv, const float* features, const int* table, int n, int budget, void* stream);
int cp_track_cost_host(const float* gallery, const float* ginv, const int* glen, const float* features, const int* slots, const float* rows,
                       int M, int S, int Tcap, int budget, int q, float* out);
int cp_track_append_host(float* gallery, float* ginv, const float* features, const int* table, int n, int budget);
int cp_linear_assignment_host(const double* cost, int rows, int cols, int ld, int* row_to_col);
/* cp_track_row_ids: the track ids of the detection slots, per row.  slots DEVICE int [capacity] as above, slot_ids DEVICE int [S * q]
 *   (the id of the track matched to each detection slot, -1: none), row_ids DEVICE int [S, M]: every entry becomes -1, then
 *   row_ids[slots[i]] = slot_ids[i] for every i < S * q with slots[i] >= 0 and slot_ids[i] >= 0.  Two launches on `stream` (fill, then
 *   scatter), no synchronisation.  Slots address distinct rows; a slot outside [0, S * M) is skipped on the device and refused by the
 *   host twin.  Checked before anything is launched: null pointers, S in 1..65535, q >= 1, M >= 0, capacity >= S * q, S * q and
 *   S * M <= 2^24.  S * M = 0 succeeds and launches nothing.  cp_track_row_ids_host: HOST only, the sequential twin. */
int cp_track_row_ids(const int* slots, const int* slot_ids, int capacity, int S, int q, int M, int* row_ids, void* stream);
int cp_track_row_ids_host(const int* slots, const int* slot_ids, int capacity, int S, int q, int M, int* row_ids);

/* ---- 3-D face alignment: similarity crops into the PRNet plan's input, position maps back to the image (face.FaceAligner) -----------
 * What PRN.process and PRN.get_landmarks do per face on the host (demo/face/prnet.py:61-127), for every candidate of every frame.  The
 * values are this library's own closed-form statement of that pipeline (csrc/face_arith.h), float32 throughout, not pinned to a
 * recording of skimage (estimate_transform / warp):
 *   candidates: cand DEVICE float32 [N,M,56] detection rows (rule.boxes = 0: the box is the min / max of the five face joints, floats
 *     5..14) or [N,M,5] boxes (x1, y1, x2, y2, score; rule.boxes = 1).  old_size = ((right - left) + bottom - top) / 2,
 *     size = (int)(old_size * expand), centre (right - (right - left) / 2, bottom - (bottom - top) / 2), x0 = cx - size / 2, y0 alike.
 *     Selected iff score > vis_thresh (strict; NaN is not), every coordinate read is finite and min_size <= size <= 32768.
 *   slots: with q = cap / N the first q selected candidates of frame n, in order, take slots n * q + 0, 1, ...
 *   crop pixel (u, v) samples the frame at (x0 + u * (size / 255), y0 + v * (size / 255)): bilinear over the four neighbours, a neighbour
 *     outside the frame contributing 0, divided by 255, channels written as R, G, B.
 *   restore: P = out * 281.6; x = P_x * (size / 255) + x0, y alike, z = P_z * (size / 255).
 * cp_face_rule (HOST): vis_thresh, expand (in (0, 1024]), min_size (1..32768), boxes.
 * cp_face_select: one wave per frame -> slots[cap] DEVICE int (n * M + m, or -1), counts[N] DEVICE int (NOT capped at q),
 *   xform[cap,3] DEVICE float32 (x0, y0, size; zeros for an unused slot).
 * cp_face_crop_frames_f32 / cp_face_crop_yuv_frames_f32: out DEVICE float32 [cap,3,256,256], every element written; zeros for a slot
 *   that is unused.  Frames are read in place through the descriptors exactly as by the re-id crops (same tables, same checks, same
 *   YUV sampler; coef: HOST int[6]).  cp_last_kernel(): face_select_kernel<rows|boxes>, face_crop_kernel<bgr|yuv|surfaces>.
 * cp_face_restore_f32: net DEVICE float32 [cap,3,256,256] (the plan's output), uv DEVICE int [2,68] (column, then row, of every
 *   landmark's cell, each in 0..255: the caller's to check) -> pos DEVICE float32 [cap,256,256,3] (NULL: not written) and
 *   landmarks DEVICE float32 [cap,68,3]; zeros for an unused slot.
 *   Checked before anything is launched (rc 1, cp_last_error): null pointers, cap in 1..256, 1 <= N <= cap, M >= 0, N * M <= 2^24, the
 *   rule's ranges, and per frame what the re-id crops check.
 * cp_face_*_host: HOST only -- sequential twins over host arrays, built from the same statements; same checks (the restore twin also
 *   refuses a uv entry outside 0..255).  What the device results are pinned to, bit for bit. */
typedef struct cp_face_rule {       /* 16 bytes */
    float vis_thresh;
    float expand;
    int min_size;
    int boxes;
} cp_face_rule;
int cp_sizeof_face_rule(void);
int cp_face_select(int N, const float* cand, int M, const void* rule, int cap, int* slots, int* counts, float* xform, void* stream);
int cp_face_crop_frames_f32(const void* table, const void* table_host, int N, int M, const int* slots, const float* xform, int cap,
                            float* out, void* stream);
int cp_face_crop_yuv_frames_f32(const void* table, const void* table_host, int N, const int* coef, int M, const int* slots,
                                const float* xform, int cap, float* out, void* stream);
int cp_face_restore_f32(const float* net, const int* slots, const float* xform, int cap, const int* uv, float* pos, float* landmarks,
                        void* stream);
int cp_face_select_host(int N, const float* cand, int M, const void* rule, int cap, int* slots, int* counts, float* xform);
int cp_face_crop_frames_host(const void* table_host, int N, int M, const int* slots, const float* xform, int cap, float* out);
int cp_face_crop_yuv_frames_host(const void* table_host, int N, const int* coef, int M, const int* slots, const float* xform, int cap,
                                 float* out);
int cp_face_restore_host(const float* net, const int* slots, const float* xform, int cap, const int* uv, float* pos, float* landmarks);

/* ---- head pose of the aligned faces (face.FaceAligner.align(pose=True) / estimate_pose) -----------------------------------------------
 * What estimate_pose and the projection of plot_pose_box do per face on the host (demo/face/utils/estimate_pose.py:67-99,
 * cv_plot.py:48-70), for every slot in two launches.  The rule is csrc/face_pose_arith.h: float64, a fixed summation order (chunks of
 * 2048 vertices, 256 lanes, a binary tree, chunks in ascending order; no atomics), a cyclic Jacobi for the rotation.
 *   src: DEVICE float32 -- from_pos = 0: the plan's output [cap,3,256,256], restored on the fly (the maps need not exist);
 *     from_pos = 1: the restored maps [cap,256,256,3].  Both give the same bits.
 *   slots / xform: as cp_face_select wrote them; a slot is used iff the restore would write it.
 *   face_ind: DEVICE int [V], cells of the flattened 256 x 256 map, each in 0..65535 (the caller's to check; a cell outside makes the
 *     slot invalid and is never read); duplicates and any order allowed.  3 <= V <= 65536.
 *   canon: DEVICE float64 [V,3], the canonical cloud minus its mean; stats: DEVICE float64 [4], that mean and rms_d1.
 *   landmarks: DEVICE float32 [cap,68,3] (cp_face_restore_f32's): landmarks 0..26 place the box.
 *   scratch: DEVICE, cp_face_pose_scratch_bytes(cap, V) bytes (0 for arguments out of range); per used slot the chunks' 13 partial
 *     moments and the pivot vertex; written before it is read, in stream order; an unused slot's part is not touched.
 *   -> P [cap,3,4] float64 ([s R | t]), angles [cap,3] float64 (matrix2angle's x, y, z), scale [cap] float64, box [cap,10,2] int
 *     (clamped to -16384..16383, truncated toward zero), valid [cap] int: 1 iff the slot is used, every vertex and moment is finite
 *     and rms_d0 > 0.  Unused and invalid slots are all zeros.
 *   Checked before anything is launched (rc 1, cp_last_error): null pointers, cap in 1..256, V in 3..65536, from_pos in {0, 1}, the
 *   scratch size.  cp_last_kernel(): face_pose_moments_kernel<net|pos>+face_pose_solve_kernel.
 * cp_face_pose_host: HOST only -- the sequential twin over host arrays, built from the same statements, same checks.  The device
 *   results equal it bit for bit except the angles (asin / atan2 / cos of two math libraries: within 1e-12 rad). */
size_t cp_face_pose_scratch_bytes(int cap, int V);
int cp_face_pose_f32(const float* src, int from_pos, const int* slots, const float* xform, int cap, const int* face_ind, int V,
                     const double* canon, const double* stats, const float* landmarks, double* scratch, size_t scratch_bytes, double* P,
                     double* angles, double* scale, int* box, int* valid, void* stream);
int cp_face_pose_host(const float* src, int from_pos, const int* slots, const float* xform, int cap, const int* face_ind, int V,
                      const double* canon, const double* stats, const float* landmarks, double* scratch, size_t scratch_bytes, double* P,
                      double* angles, double* scale, int* box, int* valid);

/* ---- the face overlays on device frames, in place (face.FaceAligner.draw) -------------------------------------------------------------
 * The content of plot_kpt, plot_vertices and plot_pose_box (demo/face/utils/cv_plot.py) by this library's own rule
 * (csrc/face_draw_arith.h: the disc and capsule statements of draw_results, k = R^2 + R), not cv2's rasteriser.  Frames and tables
 * exactly as for cp_draw_rows_frames_u8 / cp_draw_rows_yuv_frames_u8 (same descriptors, same checks; YUV: 8-bit 4:2:0 only).
 *   slots DEVICE int [cap] (a slot is used iff >= 0; frame n owns slots n * q .. n * q + q - 1, q = cap / N), landmarks DEVICE float32
 *   [cap,68,3]; box DEVICE int [cap,10,2] and valid DEVICE int [cap] (cp_face_pose_f32's; both NULL without a pose: style.pose_box
 *   must then be 0); pos DEVICE float32 [cap,256,256,3] and face_ind DEVICE int [V] (NULL unless style.vertices), 1 <= V <= 65536.
 *   A landmark / vertex sits at rint (half to even) of its x and y clamped to +-16384; a coordinate that is not finite kills its
 *   primitives.  Per face in paint order: 60 capsules k -> k + 1 (k not in 16, 21, 26, 30, 35, 41, 47, 67), 68 discs, the 13 capsules of
 *   the pose box where valid == 1.  Faces in ascending slot order, the last painter wins, opaque, clipped; the dense vertices (a disc
 *   at vertex i * vertex_step of face_ind) lie beneath all faces.  YUV: luma per pixel, chroma from the latest-painted colour among
 *   the sample's pixels; the style's colours are then (Y, U, V), converted by the caller.
 *   scratch: DEVICE, 16-byte aligned, cp_face_draw_scratch_bytes(cap) bytes (0 for cap outside 1..256).
 *   Checked before anything is launched (rc 1): null pointers, 1 <= N <= cap <= 256, radii in 0..3, vertex_step >= 1, pose_box without
 *   box / valid, vertices without pos / face_ind, V, the scratch, and per frame what draw_results checks.
 *   cp_last_kernel(): face_draw_kernel<bgr|yuv> (after face_draw_vertices_kernel<bgr|yuv> with style.vertices, and
 *   face_draw_build_kernel).
 * cp_face_draw_*_host: HOST only -- sequential painters over host arrays and host frame addresses, same statements, same checks. */
typedef struct cp_face_style {      /* 48 bytes */
    int landmarks, vertices, pose_box;                                 /* layers: 0 / 1 */
    int landmark_radius, line_radius, box_radius, vertex_radius;       /* 0..3 */
    int vertex_step;                                                   /* >= 1 */
    unsigned char colors[4][4];     /* landmark, line, vertex, box: bytes 0..2 are stored (channel order B, G, R; or Y, U, V) */
} cp_face_style;
int cp_sizeof_face_style(void);
size_t cp_face_draw_scratch_bytes(int cap);
int cp_face_draw_frames_u8(const void* table, const void* table_host, int N, const int* slots, int cap, const float* landmarks,
                           const int* box, const int* valid, const float* pos, const int* face_ind, int V, const void* style,
                           void* scratch, size_t scratch_bytes, void* stream);
int cp_face_draw_yuv_frames_u8(const void* table, const void* table_host, int N, const int* slots, int cap, const float* landmarks,
                               const int* box, const int* valid, const float* pos, const int* face_ind, int V, const void* style,
                               void* scratch, size_t scratch_bytes, void* stream);
int cp_face_draw_frames_host(const void* table_host, int N, const int* slots, int cap, const float* landmarks, const int* box,
                             const int* valid, const float* pos, const int* face_ind, int V, const void* style);
int cp_face_draw_yuv_frames_host(const void* table_host, int N, const int* slots, int cap, const float* landmarks, const int* box,
                                 const int* valid, const float* pos, const int* face_ind, int V, const void* style);

/* ---- the aligned faces rendered: z-buffer mesh rasteriser and vertex colours (face.FaceRenderer) -----------------------------------------
 * What render_texture, get_triangle_buffer and get_depth_image (demo/face/utils/render.py:85-120, 239-287; render_app.py:35-40) compute
 * per face in three nested Python loops, for every slot in three launches.  The rule is csrc/face_render_arith.h: float64 on the
 * float32 inputs; per triangle i the depth d = (float)(((z0 + z1) + z2) / 3.0) + 0.0f, the box clamped to the slot's WINDOW (the
 * reference clamps to the frame: the result is its render of any frame that contains the window, cropped to it), isPointInTri with
 * the reference's statements (a degenerate triangle covers its whole box); triangles with a coordinate that is not finite or with
 * !(d > -999999) are skipped.  The winner of a pixel is the maximum of the 64-bit key ordered(d) << 32 | (0xFFFFFFFF - i): the largest
 * depth, among equal depths the smallest index, whatever the arrival order -- the output is the same bits from run to run.
 *   pos: DEVICE float32 [cap,256,256,3] (cp_face_restore_f32's); slots: DEVICE int [cap], a slot is used iff >= 0.
 *   face_ind: DEVICE int [V] in 0..65535, 3 <= V <= 65536; tri: DEVICE int [T,3] in 0..V-1, 1 <= T <= 2^22.  Both tables are the
 *     caller's to check when it uploads them; they are not re-checked per launch.
 *   origin: DEVICE int [cap,2] = (x0, y0): image pixel (r, c) of slot s is frame pixel (x0[s] + c, y0[s] + r); a slot whose origin lies
 *     outside +-2^20 is written like an unused one.  h, w in 1..4096 with cap * h * w * 8 < 2^31.
 *   attrs: DEVICE float32 [cap,V,C], 1 <= C <= 4, or NULL: the vertices' z (C = 1; the depth image).
 *   scratch: DEVICE, 8-byte aligned, cp_face_render_scratch_bytes(cap, h, w, T) bytes (0 for arguments out of range): the keys
 *     [cap,h,w], cleared by the call itself.
 *   -> out_tri int [cap,h,w] (-1: no triangle), out_image float32 [cap,h,w,C]: (float)(((a0 + a1) + a2) / 3.0) of the winner's three
 *     vertex attributes, 0 where nothing covers.  Unused slots: all -1 / 0.
 *   Checked before anything is launched (rc 1, cp_last_error): null pointers, the ranges above, NULL attrs with C != 1, the scratch.
 *   cp_last_kernel(): face_render_clear_kernel+face_render_raster_kernel+face_render_resolve_kernel.
 * cp_face_vertex_colors_f32 / _yuv_f32: PRN.get_colors (demo/face/prnet.py:155-168) for every slot -- per vertex x clamped to
 *   [0, W-1], y to [0, H-1], rounded half to even, the frame's (B, G, R) there as float32 0..255 -> colors [cap,V,3]; zeros for a vertex
 *   with a coordinate that is not finite and for unused slots.  Frames and tables exactly as for cp_face_crop_frames_f32 /
 *   cp_face_crop_yuv_frames_f32 (same descriptors, same checks, every format word); frame n owns slots n * q .. n * q + q - 1,
 *   q = cap / N.  The frames are only read.  cp_last_kernel(): face_vertex_colors_kernel<bgr|yuv|surfaces>.
 * cp_face_*_host: HOST only -- the sequential twins over host arrays, built from the same statements, same checks; the render twin also
 *   checks face_ind and tri.  The device results equal them bit for bit. */
size_t cp_face_render_scratch_bytes(int cap, int h, int w, int T);
int cp_face_render_f32(const float* pos, const int* slots, int cap, const int* face_ind, int V, const int* tri, int T, const int* origin,
                       int h, int w, const float* attrs, int C, void* scratch, size_t scratch_bytes, int* out_tri, float* out_image,
                       void* stream);
int cp_face_render_host(const float* pos, const int* slots, int cap, const int* face_ind, int V, const int* tri, int T, const int* origin,
                        int h, int w, const float* attrs, int C, void* scratch, size_t scratch_bytes, int* out_tri, float* out_image);
int cp_face_vertex_colors_f32(const void* table, const void* table_host, int N, const float* pos, const int* slots, int cap,
                              const int* face_ind, int V, float* colors, void* stream);
int cp_face_vertex_colors_yuv_f32(const void* table, const void* table_host, int N, const int* coef, const float* pos, const int* slots,
                                  int cap, const int* face_ind, int V, float* colors, void* stream);
int cp_face_vertex_colors_host(const void* table_host, int N, const float* pos, const int* slots, int cap, const int* face_ind, int V,
                               float* colors);
int cp_face_vertex_colors_yuv_host(const void* table_host, int N, const int* coef, const float* pos, const int* slots, int cap,
                                   const int* face_ind, int V, float* colors);

/* ---- host: soft-NMS of merged results --------------------------------------------------------
 * Replaces soft_nms_39 (lib/external/nms.pyx:172-275; called from multi_pose.py:76-77).
 * boxes: HOST float32 [N,56], modified in place with the reference's quirks; keep: HOST int[N] or NULL. */
int cp_soft_nms_39(float* boxes, int N, float sigma, float Nt, float threshold, int method, int* keep, int* n_keep);

#ifdef __cplusplus
}
#endif
#endif
