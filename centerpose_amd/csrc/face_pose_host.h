// Host side of the head-pose stage: the argument checks shared by the device launcher and the host twin, and the sequential host twin
// itself (cp_face_pose_host, exported by face_pose.hip).  Plain C++ over face_pose_arith.h, no device code and no HIP header:
// tools/face_pose_host_fuzz.cpp compiles this file with the host compiler under AddressSanitizer / UBSan.  A failed check writes its
// message to `err` and returns 1.
#pragma once
#include "face_pose_arith.h"
#include "face_host.h"

inline size_t fp_scratch_bytes(int cap, int V) { return (size_t)cap * fp_slot_doubles(V) * sizeof(double); }

inline int fp_check_call(const char* who, int cap, int V, size_t scratch_bytes, char* err, size_t errn)
{
    RH_CHECK(cap >= 1 && cap <= FA_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FA_MAX_CAP);
    RH_CHECK(V >= FP_MIN_V && V <= FP_MAX_V, "%s: %d vertices outside %d..%d", who, V, FP_MIN_V, FP_MAX_V);
    RH_CHECK(scratch_bytes >= fp_scratch_bytes(cap, V), "%s: %zu bytes of scratch, %zu needed (cp_face_pose_scratch_bytes)", who,
             scratch_bytes, fp_scratch_bytes(cap, V));
    return 0;
}

// The lanes of one chunk, lane by lane and then by the tree of face_pose_arith.h -> part[13]
template <bool NET>
inline void fp_chunk_host(const float* src, const FaXform& t, const int* face_ind, int V, const double* canon, const double c[3], int chunk,
                          double part[FP_NMOM])
{
    double lanes[FP_LANES][FP_NMOM];
    for (int l = 0; l < FP_LANES; ++l) fp_lane<NET>(src, t, face_ind, V, canon, c, chunk, l, lanes[l]);
    for (int stride = FP_LANES / 2; stride >= 1; stride /= 2)
        for (int l = 0; l < stride; ++l)
            for (int k = 0; k < FP_NMOM; ++k) lanes[l][k] += lanes[l + stride][k];
    for (int k = 0; k < FP_NMOM; ++k) part[k] = lanes[0][k];
}

// Chunks in ascending order, from 0
inline void fp_combine(const double* parts, int chunks, double m[FP_NMOM])
{
    for (int k = 0; k < FP_NMOM; ++k) {
        m[k] = 0.0;
        for (int ch = 0; ch < chunks; ++ch) m[k] += parts[(size_t)ch * FP_NMOM + k];
    }
}

// HOST pose: src [cap, 3, 256, 256] (from_pos = 0: the plan's output) or [cap, 256, 256, 3] (from_pos = 1: the restored maps);
// face_ind [V], canon [V, 3] (centred), stats [4] (the canonical mean, rms_d1), landmarks [cap, 68, 3] -> scratch (per used slot the
// chunks' partial moments and the pivot; an unused slot's part is not touched), P [cap, 3, 4], angles [cap, 3], scale [cap],
// box [cap, 10, 2], valid [cap]
inline int fp_pose_host(const float* src, int from_pos, const int* slots, const float* xform, int cap, const int* face_ind, int V,
                        const double* canon, const double* stats, const float* landmarks, double* scratch, size_t scratch_bytes, double* P,
                        double* angles, double* scale, int* box, int* valid, char* err, size_t errn)
{
    const char* who = "face_pose_host";
    if (int rc = fp_check_call(who, cap, V, scratch_bytes, err, errn)) return rc;
    RH_CHECK(from_pos == 0 || from_pos == 1, "%s: source kind %d is neither 0 (net) nor 1 (pos)", who, from_pos);
    RH_CHECK(src && slots && xform && face_ind && canon && stats && landmarks && scratch && P && angles && scale && box && valid,
             "%s: null pointer", who);
    const int chunks = fp_chunks(V);
    const size_t per = fp_slot_doubles(V), map = (size_t)3 * FP_CELLS;
    for (int s = 0; s < cap; ++s) {
        FpPose o;
        FaXform t;
        if (!fh_slot(slots, xform, s, 1, FA_MAX_ROWS, &t)) {
            fp_zero(&o);
            fp_store(o, s, P, angles, scale, box, valid);
            continue;
        }
        double* parts = scratch + s * per;
        double* c = parts + (size_t)chunks * FP_NMOM;
        const float* m = src + s * map;
        if (from_pos) fp_vertex<false>(m, t, face_ind[0], c); else fp_vertex<true>(m, t, face_ind[0], c);
        for (int ch = 0; ch < chunks; ++ch) {
            if (from_pos) fp_chunk_host<false>(m, t, face_ind, V, canon, c, ch, parts + (size_t)ch * FP_NMOM);
            else fp_chunk_host<true>(m, t, face_ind, V, canon, c, ch, parts + (size_t)ch * FP_NMOM);
        }
        double mom[FP_NMOM];
        fp_combine(parts, chunks, mom);
        fp_solve(mom, c, V, stats, landmarks + (size_t)s * FA_NKPT * 3, &o);
        fp_store(o, s, P, angles, scale, box, valid);
    }
    return 0;
}
