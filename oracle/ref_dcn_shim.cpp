/* TEST INFRASTRUCTURE ONLY -- host shim that lets the reference's own DCNv2 im2col text run on a CPU.
 *
 * The Makefile cuts three pieces out of the reference's DCNv2/src/cuda/dcn_v2_im2col_cuda.cu by their
 * signature lines (the CUDA_KERNEL_LOOP macro, dmcn_im2col_bilinear and
 * modulated_deformable_im2col_gpu_kernel) into oracle/_ref/dcn_im2col_extract.inc and compiles this
 * file with -DCP_REF_EXTRACT="<that file>".  Nothing of the reference is in this file: it holds only
 * the stand-ins below and one C entry.
 *
 *   reference's compiled text : the bilinear sampler, the bounds rule, offset / mask / deformable-group
 *                               indexing, the column layout, the grid-stride loop macro
 *   stand-ins (ours)          : __device__ / __global__ -> static; blockIdx / blockDim / threadIdx /
 *                               gridDim describe one thread of one block, so the grid-stride loop walks
 *                               every index in order; the <<<...>>> launch is a plain call
 *
 * The entry takes the arguments of the reference's launcher modulated_deformable_im2col_cuda
 * (dcn_v2_im2col_cuda.cu:329-352) minus the stream and computes the same two derived values
 * (channels / deformable_group, channels * batch * height_col * width_col).
 */
#include <math.h>
#include <stddef.h>

#define __device__ static
#define __global__ static
struct cp_idx3 { int x, y, z; };
static const cp_idx3 blockIdx = {0, 0, 0}, threadIdx = {0, 0, 0}, blockDim = {1, 1, 1}, gridDim = {1, 1, 1};

#ifndef CP_REF_EXTRACT
#error "compile through oracle/Makefile: CP_REF_EXTRACT names the text cut from the reference"
#endif
#include CP_REF_EXTRACT
#ifndef CUDA_KERNEL_LOOP
#error "the extract did not define CUDA_KERNEL_LOOP"
#endif

extern "C" int cp_ref_modulated_deformable_im2col(const float *data_im, const float *data_offset, const float *data_mask,
                                                   int batch_size, int channels, int height_im, int width_im,
                                                   int height_col, int width_col, int kernel_h, int kernel_w,
                                                   int pad_h, int pad_w, int stride_h, int stride_w,
                                                   int dilation_h, int dilation_w, int deformable_group, float *data_col)
{
    if (deformable_group < 1 || channels % deformable_group)
        return 1;
    const int channel_per_deformable_group = channels / deformable_group;
    const long long total = (long long)channels * batch_size * height_col * width_col;
    if (total <= 0 || total * kernel_h * kernel_w > 0x7fffffffLL)       /* the kernel indexes with int */
        return 2;
    modulated_deformable_im2col_gpu_kernel((int)total, data_im, data_offset, data_mask, height_im, width_im, kernel_h, kernel_w,
                                           pad_h, pad_w, stride_h, stride_w, dilation_h, dilation_w,
                                           channel_per_deformable_group, batch_size, channels, deformable_group,
                                           height_col, width_col, data_col);
    return 0;
}

/* 1 when this object was compiled with floating-point contraction (the -ffp-contract=fast -mfma twin) */
extern "C" int cp_ref_contracted(void)
{
#ifdef CP_REF_CONTRACTED
    return 1;
#else
    return 0;
#endif
}
