// Head pose of the aligned faces on the device: the similarity that takes the canonical face cloud onto every slot's vertices, its Euler
// angles and the ten corners of the pose box -- what estimate_pose and plot_pose_box's projection do per face on the host after a
// download of 43 867 vertices (demo/face/utils/estimate_pose.py:67-99, cv_plot.py:48-70), for all slots in two launches.  The values
// are defined by face_pose_arith.h, float64, with a fixed summation order: the device and the host twin give the same bits up to the
// three angles (asin / atan2 / cos of two math libraries).
//
//   face_pose_moments_kernel<net|pos> : grid (chunks, cap), 256 threads.  A block adds the 13 moments of 2048 vertices of one slot: a
//                                       lane gathers its vertices (net: three planar loads of the plan's output, restored on the fly;
//                                       pos: the restored map), the lanes are combined by a tree in LDS, the partial goes to scratch.
//                                       Unused slots exit at once.
//   face_pose_solve_kernel            : grid cap, one wave.  Lanes 0..12 add the chunks' partials in ascending order, lane 0 solves
//                                       (a 3 x 3 Jacobi) and writes P, the angles, the scale, the box and valid.
//   cp_face_pose_host                 : the sequential HOST twin of face_pose_host.h, same statements
//
// No atomics; scratch is written before it is read, in stream order.  Compiled with -ffp-contract=off.
#include "common.h"
#include "face_pose_host.h"

template <bool NET>
__global__ __launch_bounds__(FP_LANES) void face_pose_moments_kernel(const float* __restrict__ src, const int* __restrict__ slots,
                                                                     const float* __restrict__ xform, const int* __restrict__ face_ind, int V,
                                                                     const double* __restrict__ canon, double* __restrict__ scratch)
{
    __shared__ double sh[FP_NMOM][FP_LANES];
    const int chunk = blockIdx.x, s = blockIdx.y, l = threadIdx.x;
    FaXform t;
    if (!fh_slot(slots, xform, s, 1, FA_MAX_ROWS, &t)) return;                 // uniform over the block
    const float* m = src + (size_t)s * 3 * FP_CELLS;
    double c[3], acc[FP_NMOM];
    fp_vertex<NET>(m, t, face_ind[0], c);
    fp_lane<NET>(m, t, face_ind, V, canon, c, chunk, l, acc);
    for (int k = 0; k < FP_NMOM; ++k) sh[k][l] = acc[k];
    __syncthreads();
    for (int stride = FP_LANES / 2; stride >= 1; stride /= 2) {
        if (l < stride)
            for (int k = 0; k < FP_NMOM; ++k) sh[k][l] += sh[k][l + stride];
        __syncthreads();
    }
    double* parts = scratch + (size_t)s * fp_slot_doubles(V);
    if (l < FP_NMOM) parts[(size_t)chunk * FP_NMOM + l] = sh[l][0];
    if (chunk == 0 && l < 3) parts[(size_t)gridDim.x * FP_NMOM + l] = c[l];
}

__global__ __launch_bounds__(CP_WAVE) void face_pose_solve_kernel(const int* __restrict__ slots, const float* __restrict__ xform, int V,
                                                                  const double* __restrict__ stats, const float* __restrict__ landmarks,
                                                                  const double* __restrict__ scratch, double* __restrict__ P,
                                                                  double* __restrict__ angles, double* __restrict__ scale, int* __restrict__ box,
                                                                  int* __restrict__ valid)
{
    __shared__ double mom[FP_NMOM];
    const int s = blockIdx.x, l = threadIdx.x, chunks = fp_chunks(V);
    FaXform t;
    const bool used = fh_slot(slots, xform, s, 1, FA_MAX_ROWS, &t);           // uniform over the wave
    const double* parts = scratch + (size_t)s * fp_slot_doubles(V);
    if (used && l < FP_NMOM) {
        double a = 0.0;
        for (int ch = 0; ch < chunks; ++ch) a += parts[(size_t)ch * FP_NMOM + l];
        mom[l] = a;
    }
    __syncthreads();
    if (l != 0) return;
    FpPose o;
    if (used) {
        double m[FP_NMOM], c[3], st[4];
        for (int k = 0; k < FP_NMOM; ++k) m[k] = mom[k];
        for (int k = 0; k < 3; ++k) c[k] = parts[(size_t)chunks * FP_NMOM + k];
        for (int k = 0; k < 4; ++k) st[k] = stats[k];
        fp_solve(m, c, V, st, landmarks + (size_t)s * FA_NKPT * 3, &o);
    } else {
        fp_zero(&o);
    }
    fp_store(o, s, P, angles, scale, box, valid);
}

extern "C" size_t cp_face_pose_scratch_bytes(int cap, int V)
{
    if (cap < 1 || cap > FA_MAX_CAP || V < FP_MIN_V || V > FP_MAX_V) return 0;
    return fp_scratch_bytes(cap, V);
}

extern "C" int cp_face_pose_host(const float* src, int from_pos, const int* slots, const float* xform, int cap, const int* face_ind, int V,
                                 const double* canon, const double* stats, const float* landmarks, double* scratch, size_t scratch_bytes,
                                 double* P, double* angles, double* scale, int* box, int* valid)
{
    char err[256];
    err[0] = 0;
    if (int rc = fp_pose_host(src, from_pos, slots, xform, cap, face_ind, V, canon, stats, landmarks, scratch, scratch_bytes, P, angles, scale,
                              box, valid, err, sizeof(err))) {
        cp_set_error("%s", err);
        return rc;
    }
    return 0;
}

// face_ind DEVICE int [V], every entry in 0..65535: checked by the caller (face.FaceAligner) when it is uploaded; a cell outside the
// map makes the slot invalid, it is never read.
extern "C" int cp_face_pose_f32(const float* src, int from_pos, const int* slots, const float* xform, int cap, const int* face_ind, int V,
                                const double* canon, const double* stats, const float* landmarks, double* scratch, size_t scratch_bytes,
                                double* P, double* angles, double* scale, int* box, int* valid, void* stream)
{
    const char* who = "face_pose";
    char err[256];
    err[0] = 0;
    if (int rc = fp_check_call(who, cap, V, scratch_bytes, err, sizeof(err))) {
        cp_set_error("%s", err);
        return rc;
    }
    CP_CHECK_ARG(from_pos == 0 || from_pos == 1, "%s: source kind %d is neither 0 (net) nor 1 (pos)", who, from_pos);
    CP_CHECK_ARG(src && slots && xform && face_ind && canon && stats && landmarks && scratch && P && angles && scale && box && valid,
                 "%s: null pointer", who);
    const dim3 grid((unsigned)fp_chunks(V), (unsigned)cap);
    if (from_pos)
        hipLaunchKernelGGL(face_pose_moments_kernel<false>, grid, dim3(FP_LANES), 0, (hipStream_t)stream, src, slots, xform, face_ind, V, canon,
                           scratch);
    else
        hipLaunchKernelGGL(face_pose_moments_kernel<true>, grid, dim3(FP_LANES), 0, (hipStream_t)stream, src, slots, xform, face_ind, V, canon,
                           scratch);
    CP_CHECK_LAUNCH("face_pose_moments_kernel");
    hipLaunchKernelGGL(face_pose_solve_kernel, dim3((unsigned)cap), dim3(CP_WAVE), 0, (hipStream_t)stream, slots, xform, V, stats, landmarks,
                       scratch, P, angles, scale, box, valid);
    CP_CHECK_LAUNCH("face_pose_solve_kernel");
    cp_note_kernel(from_pos ? "face_pose_moments_kernel<pos>+face_pose_solve_kernel" : "face_pose_moments_kernel<net>+face_pose_solve_kernel");
    return 0;
}
