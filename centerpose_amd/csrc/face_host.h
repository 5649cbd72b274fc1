// Host side of the 3-D face stage: the argument checks shared by the device launchers and the host twins, and the sequential host
// twins themselves (cp_face_select_host / cp_face_crop_frames_host / cp_face_crop_yuv_frames_host / cp_face_restore_host, exported by
// face_stage.hip).  Plain C++ over face_arith.h and the descriptor mirrors, samplers and frame checks of reid_host.h, no device code
// and no HIP header: tools/face_host_fuzz.cpp compiles this file with the host compiler under AddressSanitizer / UBSan.  A failed
// check writes its message to `err` and returns 1.
#pragma once
#include "face_arith.h"
#include "reid_host.h"

// the selection's parameters (mirror of cp_face_rule, include/centerpose_hip.h)
struct FhRule { float vis_thresh, expand; int min_size, boxes; };
static_assert(sizeof(FhRule) == 16, "cp_face_rule is 16 bytes");

inline int fh_check_call(const char* who, int N, int M, int cap, char* err, size_t errn)
{
    RH_CHECK(cap >= 1 && cap <= FA_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FA_MAX_CAP);
    RH_CHECK(N >= 1, "%s: %d frames: at least one", who, N);
    RH_CHECK(N <= cap, "%s: %d frames for a capacity of %d: every frame needs a slot", who, N, cap);
    RH_CHECK(M >= 0, "%s: negative candidate count %d", who, M);
    RH_CHECK((long long)N * M <= FA_MAX_ROWS, "%s: %d x %d candidates are too many for one call (at most %d)", who, N, M, FA_MAX_ROWS);
    return 0;
}

inline int fh_check_rule(const char* who, const FhRule* r, char* err, size_t errn)
{
    RH_CHECK(r, "%s: null rule", who);
    RH_CHECK(r->boxes == 0 || r->boxes == 1, "%s: candidate kind %d is neither 0 (rows) nor 1 (boxes)", who, r->boxes);
    RH_CHECK(r->min_size >= 1 && r->min_size <= FA_MAX_SIZE, "%s: min_size %d outside 1..%d", who, r->min_size, FA_MAX_SIZE);
    RH_CHECK(r->expand > 0.f && r->expand <= 1024.f, "%s: expand %g outside (0, 1024]", who, (double)r->expand);
    return 0;
}

// HOST selection: slots[cap] (n * M + m of the first q = cap / N selected candidates of frame n at n * q + 0, 1, ...; -1: unused),
// counts[N] (selected candidates per frame, uncapped), xform[cap] (zeros for an unused slot)
inline int fh_select_host(int N, const float* cand, int M, const FhRule* rule, int cap, int* slots, int* counts, float* xform, char* err,
                          size_t errn)
{
    const char* who = "face_select_host";
    if (int rc = fh_check_call(who, N, M, cap, err, errn)) return rc;
    if (int rc = fh_check_rule(who, rule, err, errn)) return rc;
    RH_CHECK(slots && counts && xform && (cand || M == 0), "%s: null pointer", who);
    const int q = cap / N, stride = rule->boxes ? FA_BOX : FA_ROW;
    for (int s = 0; s < cap; ++s) {
        slots[s] = -1;
        xform[3 * s] = xform[3 * s + 1] = xform[3 * s + 2] = 0.f;
    }
    for (int n = 0; n < N; ++n) {
        int c = 0;
        for (int m = 0; m < M; ++m) {
            FaXform t;
            if (!fa_select(cand + ((size_t)n * M + m) * stride, rule->boxes, rule->vis_thresh, rule->expand, rule->min_size, &t)) continue;
            if (c < q) {
                const int s = n * q + c;
                slots[s] = n * M + m;
                xform[3 * s] = t.x0; xform[3 * s + 1] = t.y0; xform[3 * s + 2] = t.size;
            }
            ++c;
        }
        counts[n] = c;
    }
    return 0;
}

// a slot's crop square as the crop and restore launches read it back; false: the slot is written as zeros
FA_HD bool fh_slot(const int* slots, const float* xform, int s, int N, int M, FaXform* t)
{
    const int idx = slots[s];
    if (idx < 0 || idx >= N * M) return false;
    t->x0 = xform[3 * s]; t->y0 = xform[3 * s + 1]; t->size = xform[3 * s + 2];
    return t->size >= 1.f && t->size <= (float)FA_MAX_SIZE;       // (NaN fails)
}

// HOST crops: out [cap, 3, 256, 256]; a slot that is unused or out of range is written as zeros
template <class Desc, class Make>
inline void fh_crop(const Desc* table, int N, int M, const int* slots, const float* xform, int cap, float* out, Make make)
{
    const size_t plane = (size_t)FA_RES * FA_RES;
    for (int s = 0; s < cap; ++s) {
        float* o = out + (size_t)s * 3 * plane;
        FaXform t;
        if (!fh_slot(slots, xform, s, N, M, &t)) {
            for (size_t i = 0; i < 3 * plane; ++i) o[i] = 0.f;
            continue;
        }
        const Desc& d = table[slots[s] / M];
        const auto src = make(d);
        for (int v = 0; v < FA_RES; ++v)
            for (int u = 0; u < FA_RES; ++u) {
                float r[3];
                fa_pixel(src, d.H, d.W, t, v, u, r);
                for (int k = 0; k < 3; ++k) o[k * plane + (size_t)v * FA_RES + u] = r[k];
            }
    }
}

inline int fh_crop_frames_host(const RhFrameDesc* table, int N, int M, const int* slots, const float* xform, int cap, float* out, char* err,
                               size_t errn)
{
    const char* who = "face_crop_frames_host";
    if (int rc = fh_check_call(who, N, M, cap, err, errn)) return rc;
    RH_CHECK(table && slots && xform && out, "%s: null pointer", who);
    if (int rc = rh_check_frames(who, table, N, err, errn)) return rc;
    fh_crop(table, N, M, slots, xform, cap, out, [](const RhFrameDesc& d) { return rh_source(d); });
    return 0;
}

inline int fh_crop_yuv_frames_host(const RhYuvFrameDesc* table, int N, const int* coef, int M, const int* slots, const float* xform, int cap,
                                   float* out, char* err, size_t errn)
{
    const char* who = "face_crop_yuv_frames_host";
    if (int rc = fh_check_call(who, N, M, cap, err, errn)) return rc;
    RH_CHECK(table && slots && xform && out, "%s: null pointer", who);
    if (int rc = rh_check_yuv_frames(who, table, N, coef, err, errn)) return rc;
    const YfCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    fh_crop(table, N, M, slots, xform, cap, out, [&](const RhYuvFrameDesc& d) { return rh_yuv_source<true>(d, k); });
    return 0;
}

inline int fh_check_uv(const char* who, const int* uv, char* err, size_t errn)
{
    RH_CHECK(uv, "%s: null uv_kpt_ind", who);
    for (int i = 0; i < 2 * FA_NKPT; ++i)
        RH_CHECK(uv[i] >= 0 && uv[i] < FA_RES, "%s: uv_kpt_ind[%d][%d] = %d outside 0..%d", who, i / FA_NKPT, i % FA_NKPT, uv[i], FA_RES - 1);
    return 0;
}

// HOST restore: net [cap, 3, 256, 256] (the plan's output) -> pos [cap, 256, 256, 3] (may be null: landmarks only) and
// landmarks [cap, 68, 3]; a slot that is unused is written as zeros.  uv [2][68]: column, then row, of every landmark's cell.
inline int fh_restore_host(const float* net, const int* slots, const float* xform, int cap, const int* uv, float* pos, float* landmarks,
                           char* err, size_t errn)
{
    const char* who = "face_restore_host";
    RH_CHECK(cap >= 1 && cap <= FA_MAX_CAP, "%s: capacity %d outside 1..%d", who, cap, FA_MAX_CAP);
    RH_CHECK(net && slots && xform && landmarks, "%s: null pointer", who);
    if (int rc = fh_check_uv(who, uv, err, errn)) return rc;
    const size_t plane = (size_t)FA_RES * FA_RES;
    for (int s = 0; s < cap; ++s) {
        const float* o = net + (size_t)s * 3 * plane;
        FaXform t;
        const bool live = fh_slot(slots, xform, s, 1, FA_MAX_ROWS, &t);
        if (pos)
            for (size_t c = 0; c < plane; ++c) {
                float r[3] = {0.f, 0.f, 0.f};
                if (live) fa_restore(t, o[c], o[plane + c], o[2 * plane + c], r);
                for (int k = 0; k < 3; ++k) pos[((size_t)s * plane + c) * 3 + k] = r[k];
            }
        for (int j = 0; j < FA_NKPT; ++j) {
            const size_t c = (size_t)uv[FA_NKPT + j] * FA_RES + uv[j];
            float r[3] = {0.f, 0.f, 0.f};
            if (live) fa_restore(t, o[c], o[plane + c], o[2 * plane + c], r);
            for (int k = 0; k < 3; ++k) landmarks[((size_t)s * FA_NKPT + j) * 3 + k] = r[k];
        }
    }
    return 0;
}
