"""Deterministic synthetic inputs shared by the parity tests and tests/golden/make_golden.py.

numpy RandomState only (bit-stable across numpy versions and machines), so the GPU box regenerates
exactly the inputs the golden outputs were produced from.
"""
import numpy as np

F32 = np.float32


def sigmoid(x):
    return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(F32)


def decode_random(seed, B=2, H=128, W=128, J=17):
    """SURVEY 8d decode-only fixture inputs: hm = sigmoid(N(0,1)), hm_hp = sigmoid(N(-1,1)),
    wh ~ U(0,30), hps ~ N(0,8), reg / hp_offset ~ U(0,1)."""
    r = np.random.RandomState(seed)
    hm = sigmoid(r.randn(B, 1, H, W))
    hm_hp = sigmoid(r.randn(B, J, H, W) - 1.0)
    wh = (r.rand(B, 2, H, W) * 30).astype(F32)
    hps = (r.randn(B, 2 * J, H, W) * 8).astype(F32)
    reg = r.rand(B, 2, H, W).astype(F32)
    hp_offset = r.rand(B, 2, H, W).astype(F32)
    return dict(hm=hm, wh=wh, hps=hps, reg=reg, hm_hp=hm_hp, hp_offset=hp_offset)


def decode_people(seed, B=2, H=128, W=128, J=17, n_people=7):
    """Structured case: a few planted people.  Centre / joint heat maps are sums of Gaussian
    blobs on a low noise floor (so fewer than K peaks exceed 0.1: exercises the -1 / -10000
    sentinels), hps points from each centre to its joints (so candidates are accepted), some
    joints are pushed outside the box (rejection path), wh is the person's extent."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    hm = np.full((B, 1, H, W), 0.0, np.float64)
    hm_hp = np.full((B, J, H, W), 0.0, np.float64)
    wh = np.zeros((B, 2, H, W), np.float64)
    hps = np.zeros((B, 2 * J, H, W), np.float64)
    for b in range(B):
        for _ in range(n_people):
            cy, cx = r.randint(12, H - 12), r.randint(12, W - 12)
            bw, bh = r.uniform(8, 30), r.uniform(10, 40)
            amp = r.uniform(0.3, 0.95)
            hm[b, 0] = np.maximum(hm[b, 0], amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.7 ** 2)))
            wh[b, 0, cy - 2:cy + 3, cx - 2:cx + 3] = bw
            wh[b, 1, cy - 2:cy + 3, cx - 2:cx + 3] = bh
            for j in range(J):
                jy = cy + r.uniform(-0.45, 0.45) * bh
                jx = cx + r.uniform(-0.45, 0.45) * bw
                if r.rand() < 0.15:          # outside the box -> rejected, regression kept
                    jx = cx + bw * 0.8
                jy = float(np.clip(jy, 1, H - 2)); jx = float(np.clip(jx, 1, W - 2))
                hps[b, 2 * j, cy - 2:cy + 3, cx - 2:cx + 3] = jx - cx + r.uniform(-1.5, 1.5)
                hps[b, 2 * j + 1, cy - 2:cy + 3, cx - 2:cx + 3] = jy - cy + r.uniform(-1.5, 1.5)
                a = r.uniform(0.05, 0.9)     # some below the 0.1 threshold
                if b == B - 1 and j >= J - 2:
                    a = r.uniform(0.03, 0.07)  # no valid candidate at all -> score -1 for every person
                hm_hp[b, j] = np.maximum(hm_hp[b, j], a * np.exp(-((yy - jy) ** 2 + (xx - jx) ** 2) / (2 * 1.3 ** 2)))
    # strictly positive, tie-free noise floor well below 0.1
    def floor(shape):   # distinct values per plane: a scaled random permutation
        out = np.empty(shape, np.float64)
        for idx in np.ndindex(shape[:2]):
            out[idx] = ((r.permutation(H * W) + 1.0) / (H * W) * 2e-2).reshape(H, W)
        return out
    hm = hm + floor(hm.shape)
    hm_hp = hm_hp + floor(hm_hp.shape)
    reg = r.rand(B, 2, H, W)
    hp_offset = r.rand(B, 2, H, W)
    return dict(hm=hm.astype(F32), wh=wh.astype(F32), hps=hps.astype(F32), reg=reg.astype(F32),
                hm_hp=hm_hp.astype(F32), hp_offset=hp_offset.astype(F32))


def assert_tie_free(scores_sorted, what):
    """strict gaps inside the top-K and to rank K+1 (torch.topk tie order is unspecified)."""
    d = np.diff(scores_sorted.astype(np.float64), axis=-1)
    assert (d < 0).all(), "%s: ties inside top-K+1" % what


DECODE_CASES = {
    # name: (generator, kwargs, K, use_reg, use_hp_offset)
    "rand_b2": (decode_random, dict(seed=317, B=2), 100, True, True),
    "rand_b1_noreg": (decode_random, dict(seed=11, B=1), 100, False, False),
    "rand_small": (decode_random, dict(seed=5, B=3, H=32, W=48), 40, True, True),
    "rand_ragged": (decode_random, dict(seed=7, B=1, H=40, W=24, J=5), 17, True, False),
    "people_b2": (decode_people, dict(seed=3, B=2), 100, True, True),
    # maps above 32768 keys per plane (the multi-block select path): FIX_RES=false inputs, e.g. hrnet_w32_512.yaml
    # TEST_SCALES [1,2] puts a 640x480 image at scale 2 on a 248x328 map (base_detector.py:42-43)
    "rand_256": (decode_random, dict(seed=26, B=1, H=256, W=256), 100, True, True),
    "rand_248x328": (decode_random, dict(seed=29, B=2, H=248, W=328), 100, True, True),
    "people_248x328": (decode_people, dict(seed=31, B=1, H=248, W=328, n_people=12), 100, True, False),
}


def flip_inputs(seed=41, H=12, W=20, J=17):
    """Batch of 2 (image, mirrored twin) head outputs for the flip-test merge (multi_pose.py:45-53)."""
    r = np.random.RandomState(seed)
    return dict(hm=sigmoid(r.randn(2, 1, H, W)), wh=(r.rand(2, 2, H, W) * 30).astype(F32),
                hps=(r.randn(2, 2 * J, H, W) * 8).astype(F32), reg=r.rand(2, 2, H, W).astype(F32),
                hm_hp=sigmoid(r.randn(2, J, H, W) - 1.0), hp_offset=r.rand(2, 2, H, W).astype(F32))


# ---------------------------------------------------------------------------------------------------------------------
# DCNv2 inputs.  Shared by the GPU kernel tests (tests/test_conv_hip.py), the reference pin (tests/test_dcn_reference_pin.py)
# and tests/golden/make_golden_dcn.py, so that the committed reference outputs belong to exactly the inputs the kernel sees.
# The seeds and the order of the draws are those the GPU tests have always used.

def _dcn_case(seed, B, C, Co, H, W, big_offsets):
    r = np.random.RandomState(seed)
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, 3, 3) / (3 * C ** 0.5)).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 18, H, W) * (4.0 if big_offsets else 1.0)).astype(np.float32)
    if big_offsets:                     # far out-of-range and exactly-on-boundary samples
        off[0, :, 0, 0] = 3 * H
        off[0, :, 1, 1] = -3 * H
        off[-1, 0::2, 2, 2] = -1.0      # h_im == integer boundary rows
        off[-1, 1::2, 2, 3] = W
    m = r.rand(B, 9, H, W).astype(np.float32)
    return x, w, b, off, m


def _dcn_mask_logits(seed, shape):
    """Mask LOGITS for the om_sigmoid=True mode -- the mode every in-plan launch runs (engine.emit_dcn; the reference applies
    torch.sigmoid to the mask third of conv_offset_mask's output, DCNv2/dcn_v2.py:117-127, then calls dcn_v2_forward): normal
    logits plus saturating ones (|logit| > 20, +-90: exp overflows / underflows in float32).  -> (logits, sigmoid(logits)) with
    the sigmoid evaluated by torch in float32 like the reference."""
    import torch
    r = np.random.RandomState(seed + 1000)
    lg = (r.randn(*shape) * 3.0).astype(np.float32)
    flat = lg.reshape(-1)
    flat[0::17] = 25.0
    flat[1::19] = -25.0
    flat[2::23] = 90.0
    flat[3::29] = -90.0
    flat[4::31] = 0.0
    return lg, torch.sigmoid(torch.from_numpy(lg)).numpy()


def dcn_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def _dcn_dict(x, w, b, off, m, args=(3, 3, 1, 1, 1, 1, 1, 1, 1), logits=None, relu=False, **extra):
    """x, w, b, off, m: what dcn_v2_forward takes (m is the mask itself); args = (kh, kw, sh, sw, ph, pw, dh, dw, dg); logits: the
    mask logits when the kernel test runs the sigmoid-inside mode; relu: the kernel test compares max(ref, 0)."""
    return dict(x=x, w=w, b=b, off=off, m=m, args=tuple(int(a) for a in args), logits=logits, relu=relu, **extra)


# test_dcn_v2_vs_scalar_oracle: (C, Co, H, W, big, tile)
DCN_KERNEL_SHAPES = [(16, 64, 12, 10, True, 0), (64, 64, 16, 16, False, 128064), (32, 32, 9, 13, True, 128032), (128, 128, 8, 8, False, 64064),
                     (64, 64, 11, 13, True, 64064), (32, 128, 9, 16, False, 64128), (16, 64, 9, 7, True, 64064), (48, 128, 6, 10, True, 64128),
                     (128, 256, 8, 8, False, 64128), (32, 64, 12, 12, True, 128064), (96, 128, 6, 10, True, 64032), (48, 64, 5, 9, True, 64032),
                     (128, 64, 11, 13, True, 0), (256, 64, 5, 6, True, 0)]
# test_dcn_v2_split_k_vs_scalar_oracle: (C, Co, H, W, S, tile)
DCN_SPLITK_SHAPES = [(64, 64, 9, 7, 3, 0), (32, 128, 6, 10, 9, 64128), (128, 256, 8, 8, 3, 64064), (48, 64, 5, 9, 2, 0)]
# test_dcn_v2_kernel_deformable_groups_vs_scalar_oracle: (C, Co, dg, tile, S)
DCN_KERNEL_DG_SHAPES = [(64, 64, 2, 0, 1), (128, 128, 4, 64128, 1), (64, 64, 2, 0, 3), (96, 64, 3, 128064, 1)]
# test_dcn_v2_forward_deformable_groups: (C, Co, dg, k, s, p, d)
DCN_FORWARD_DG_ROWS = [(32, 64, 2, 3, 1, 1, 1), (64, 64, 4, 3, 1, 1, 1), (96, 128, 2, 3, 2, 1, 1), (12, 7, 3, 3, 1, 2, 2),
                       (20, 40, 2, 1, 1, 0, 1), (64, 32, 1, 3, 1, 1, 1)]
# test_dcn_v2_forward_full_argument_space: (C, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg)
DCN_FULL_ARG_ROWS = [(16, 24, 3, 3, 2, 1, 1, 2, 1, 2, 1), (32, 16, 1, 3, 1, 2, 0, 1, 1, 1, 2), (8, 12, 5, 5, 1, 1, 2, 2, 1, 1, 1),
                     (16, 8, 3, 5, 2, 2, 3, 1, 2, 1, 1), (16, 16, 7, 7, 1, 1, 3, 3, 1, 1, 1)]


def dcn_kernel_case(C, Co, H, W, big, tile=0, sig=False):
    """Inputs of test_dcn_v2_vs_scalar_oracle[sig]."""
    x, w, b, off, m = _dcn_case(C + H, 2, C, Co, H, W, big)
    lg = None
    if sig:
        lg, m = _dcn_mask_logits(C + H, m.shape)
    return _dcn_dict(x, w, b, off, m, logits=lg, tile=tile)


def dcn_splitk_case(C, Co, H, W, S, tile=0, sig=False):
    """Inputs of test_dcn_v2_split_k_vs_scalar_oracle (compared after ReLU)."""
    x, w, b, off, m = _dcn_case(C + S, 2, C, Co, H, W, True)
    lg = None
    if sig:
        lg, m = _dcn_mask_logits(C + S, m.shape)
    return _dcn_dict(x, w, b, off, m, logits=lg, relu=True, tile=tile, S=S)


def dcn_kernel_dg_case(C, Co, dg, tile=0, S=1):
    """Inputs of test_dcn_v2_kernel_deformable_groups_vs_scalar_oracle (mask logits, compared after ReLU)."""
    r = np.random.RandomState(C + dg + S)
    B, H, W, kk = 2, 9, 12, 9
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, 3, 3) / (3 * C ** 0.5)).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * dg * kk, H, W) * 3.0).astype(np.float32)
    lg, m = _dcn_mask_logits(C + dg, (B, dg * kk, H, W))
    return _dcn_dict(x, w, b, off, m, (3, 3, 1, 1, 1, 1, 1, 1, dg), logits=lg, relu=True, tile=tile, S=S)


def dcn_forward_dg_case(C, Co, dg, k, s, p, d):
    """Inputs of test_dcn_v2_forward_deformable_groups."""
    r = np.random.RandomState(C * 3 + dg)
    B, H, W = 2, 10, 13
    Ho, Wo = dcn_out_hw(H, W, k, k, s, s, p, p, d, d)
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, k, k) * 0.2).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * dg * k * k, Ho, Wo) * 2.5).astype(np.float32)
    off[0, :, 0, 0] = 3 * H                     # far out of range in every group
    off[-1, 0::2, 1, 1] = -1.0                  # on the boundary rule
    m = r.rand(B, dg * k * k, Ho, Wo).astype(np.float32)
    return _dcn_dict(x, w, b, off, m, (k, k, s, s, p, p, d, d, dg))


def dcn_full_arg_case(C, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg):
    """Inputs of test_dcn_v2_forward_full_argument_space."""
    r = np.random.RandomState(C + 3 * kh + 5 * kw + sh)
    B, H, W = 2, 12, 15
    Ho, Wo = dcn_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    kk = kh * kw
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, kh, kw) * 0.2).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * dg * kk, Ho, Wo) * 2.0).astype(np.float32)
    off[0, :, 0, 0] = 4 * H
    off[-1, 0::2, -1, -1] = -1.0
    m = r.rand(B, dg * kk, Ho, Wo).astype(np.float32)
    return _dcn_dict(x, w, b, off, m, (kh, kw, sh, sw, ph, pw, dh, dw, dg))


def dcn_gpu_fuzz_cases():
    """The 24 cases of test_dcn_v2_forward_random_argument_fuzz, in its order."""
    r = np.random.RandomState(2024)
    out = []
    while len(out) < 24:
        dg = int(r.choice([1, 1, 2, 3]))
        C = dg * int(r.choice([4, 8, 16, 24]))
        Co = int(r.choice([3, 8, 17, 40]))
        kh, kw = int(r.randint(1, 6)), int(r.randint(1, 6))
        sh, sw = int(r.randint(1, 4)), int(r.randint(1, 4))
        ph, pw = int(r.randint(0, 4)), int(r.randint(0, 4))
        dh, dw = int(r.randint(1, 3)), int(r.randint(1, 3))
        B, H, W = 2, int(r.randint(7, 15)), int(r.randint(7, 15))
        Ho, Wo = dcn_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
        if Ho < 1 or Wo < 1:
            continue
        kk = kh * kw
        x = r.randn(B, C, H, W).astype(np.float32)
        w = (r.randn(Co, C, kh, kw) / np.sqrt(C * kk)).astype(np.float32)
        b = r.randn(Co).astype(np.float32)
        off = (r.randn(B, 2 * dg * kk, Ho, Wo) * 1.5).astype(np.float32)
        m = r.rand(B, dg * kk, Ho, Wo).astype(np.float32)
        out.append(_dcn_dict(x, w, b, off, m, (kh, kw, sh, sw, ph, pw, dh, dw, dg)))
    return out


def dcn_pin_fuzz_cases(n=240, seed=950):
    """Seeded fuzz of the reference pin: kh, kw 1..5, stride 1..3, pad 0..3, dilation 1..3 per axis, dg 1..4, odd maps, B 1..3;
    offsets N(0, 2.5) with a few far / on-the-lattice values, masks with exact 0 and 1."""
    r = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        dg = int(r.randint(1, 5))
        C = dg * int(r.choice([1, 2, 3, 5]))
        Co = int(r.choice([1, 3, 8, 13]))
        kh, kw = int(r.randint(1, 6)), int(r.randint(1, 6))
        sh, sw = int(r.randint(1, 4)), int(r.randint(1, 4))
        ph, pw = int(r.randint(0, 4)), int(r.randint(0, 4))
        dh, dw = int(r.randint(1, 4)), int(r.randint(1, 4))
        B, H, W = int(r.randint(1, 4)), 2 * int(r.randint(2, 8)) + 1, 2 * int(r.randint(2, 8)) + 1
        Ho, Wo = dcn_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
        if Ho < 1 or Wo < 1:
            continue
        kk = kh * kw
        x = r.randn(B, C, H, W).astype(np.float32)
        w = (r.randn(Co, C, kh, kw) / np.sqrt(C * kk)).astype(np.float32)
        b = r.randn(Co).astype(np.float32)
        off = (r.randn(B, 2 * dg * kk, Ho, Wo) * 2.5).astype(np.float32)
        flat = off.reshape(-1)
        flat[0::13] = np.round(flat[0::13])          # integer offsets: samples exactly on the lattice and on the -1 / H lines
        flat[1::37] = np.float32(3 * H)
        flat[2::41] = np.float32(-1e6)
        flat[3::43] = np.float32(-0.0)
        m = r.rand(B, dg * kk, Ho, Wo).astype(np.float32)
        m.reshape(-1)[0::11] = 0.0
        m.reshape(-1)[1::11] = 1.0
        out.append(_dcn_dict(x, w, b, off, m, (kh, kw, sh, sw, ph, pw, dh, dw, dg)))
    return out


# --- boundary lattice ------------------------------------------------------------------------------------------------
# (name, stride, pad, dilation, dg): 3 x 3 taps on a 7 x 9 map
DCN_LATTICE_CONFIGS = [("s1p1d1", 1, 1, 1, 1), ("s2p0d1", 2, 0, 1, 1), ("s2p2d1", 2, 2, 1, 1), ("s1p2d2", 1, 2, 2, 1),
                       ("s2p0d2", 2, 0, 2, 1), ("s2p2d2", 2, 2, 2, 1), ("s1p1d1g2", 1, 1, 1, 2), ("s2p2d2g2", 2, 2, 2, 2)]
DCN_LATTICE_HW = (7, 9)


def dcn_lattice_targets(N):
    """(label, coordinate, side) the sampling coordinate h_im (w_im) has to land on, for an axis of N rows (columns).  side 0: hit
    it exactly; side +1 / -1: the float just above / below it.  These are the points where the reference's conditions switch
    (dcn_v2_im2col_cuda.cu:28-48,180): `> -1`, `floor`, `h_low >= 0`, `h_high <= height - 1`, `< height`."""
    N = float(N)
    return [("-1", -1.0, 0), ("-1+", -1.0, +1), ("-0.5", -0.5, 0), ("0-", 0.0, -1), ("0", 0.0, 0), ("int", 2.0, 0), ("frac", 2.25, 0),
            ("N-1", N - 1, 0), ("N-0.5", N - 0.5, 0), ("N-", N, -1), ("N", N, 0), ("N+0.5", N + 0.5, 0),
            ("+3N", 3 * N, 0), ("-3N", -3 * N, 0), ("+1e6", 1e6, 0), ("-1e6", -1e6, 0)]


def dcn_lattice_offset(base, t, side):
    """The float32 offset that puts float32(base) + offset -- the reference's `h_in + i * dilation_h + offset_h`, an int plus a
    float evaluated in float32 -- on the target: exactly on t (side 0; every t of the list is reachable exactly for |base| < 32), or
    on the nearest reachable float strictly above (side +1) / below (side -1) t.  The sum is rounded, so for base != 0 the nearest
    reachable neighbour of t can be a few ulps of t away."""
    f = np.float32
    base = f(base)
    off = f(f(t) - base)
    if side == 0:
        assert f(base + off) == f(t), (base, t)
        if base == 0 and t == 0:
            off = f(-0.0)                # the -0.0 offset of the list: 0 + -0.0 is +0.0 in the reference's arithmetic
        return off
    for e in range(-100, 0):             # the smallest power-of-two step away from t that survives both roundings
        off = f(float(t) + side * 2.0 ** e - float(base))
        got = f(base + off)
        if (side > 0 and got > f(t)) or (side < 0 and got < f(t)):
            return off
    raise AssertionError((base, t, side))


def dcn_lattice_case(name, s, p, d, dg):
    """Every 3 x 3 tap of every output position aims at one (h, w) target pair: each h target with an interior w (2.25), each w
    target with an interior h, and each h target with the same-named w target (both conditions at once).  Batch images are added
    until every pair has a position.  Distinct weight per (o, c, i, j), masks 0 / 1 / random.  Returns the case and, in
    `h_im` / `w_im` [B, 9, Ho, Wo], the float32 coordinates the reference's expression evaluates to."""
    H, W = DCN_LATTICE_HW
    k, kk = 3, 9
    Ho, Wo = dcn_out_hw(H, W, k, k, s, s, p, p, d, d)
    th, tw = dcn_lattice_targets(H), dcn_lattice_targets(W)
    inner = ("frac", 2.25, 0)
    pairs = [(a, inner) for a in th] + [(inner, b) for b in tw] + list(zip(th, tw))
    # which position aims at which pair: a "just above / below" target goes where some tap's integer part is 0 or -1 on that axis
    # (there the exact float neighbour of the target is reachable), the rest fill up; images are added until every pair has a place
    def near(q, n_out):
        return [v for v in range(n_out) if any(v * s - p + i * d in (0, -1) for i in range(k))]
    ys_ok, xs_ok = near(0, Ho), near(0, Wo)
    place = {}
    order = sorted(range(len(pairs)), key=lambda a: -(abs(pairs[a][0][2]) + abs(pairs[a][1][2])))
    B = 0
    for a in order:
        (_, _, s_h), (_, _, s_w) = pairs[a]
        pos = None
        while pos is None:
            free = [q for q in range(B * Ho * Wo) if q not in place]
            good = [q for q in free if (not s_h or (q // Wo) % Ho in ys_ok) and (not s_w or q % Wo in xs_ok)]
            if good:
                pos = good[0]
            else:
                B += 1
        place[pos] = a
    for q in range(B * Ho * Wo):
        place.setdefault(q, q % len(pairs))
    C, Co = 2 * dg, 5
    r = np.random.RandomState(7000 + 100 * s + 10 * p + d + 1000 * dg)
    x = r.randn(B, C, H, W).astype(np.float32)
    w = ((np.arange(Co * C * kk, dtype=np.float64).reshape(Co, C, k, k) % 89 - 44) / 64 + r.rand(Co, C, k, k) / 256).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = np.zeros((B, dg, kk, 2, Ho, Wo), np.float32)
    h_im = np.zeros((B, dg, kk, Ho, Wo), np.float32)
    w_im = np.zeros((B, dg, kk, Ho, Wo), np.float32)
    for pos in range(B * Ho * Wo):
        bi, y, xx = pos // (Ho * Wo), (pos // Wo) % Ho, pos % Wo
        for g in range(dg):
            (_, t_h, s_h), (_, t_w, s_w) = pairs[(place[pos] + g * (len(th) + 1)) % len(pairs)]     # the groups aim at different targets
            for i in range(k):
                for j in range(k):
                    bh, bw = y * s - p + i * d, xx * s - p + j * d
                    oh, ow = dcn_lattice_offset(bh, t_h, s_h), dcn_lattice_offset(bw, t_w, s_w)
                    off[bi, g, i * k + j, 0, y, xx], off[bi, g, i * k + j, 1, y, xx] = oh, ow
                    h_im[bi, g, i * k + j, y, xx] = np.float32(bh) + oh
                    w_im[bi, g, i * k + j, y, xx] = np.float32(bw) + ow
    m = (0.25 + 0.75 * r.rand(B, dg * kk, Ho, Wo)).astype(np.float32)
    m.reshape(-1)[0::29] = 0.0
    m.reshape(-1)[1::7] = 1.0
    return _dcn_dict(x, w, b, off.reshape(B, 2 * dg * kk, Ho, Wo), m, (k, k, s, s, p, p, d, d, dg), name=name,
                     h_im=h_im.reshape(B, dg * kk, Ho, Wo), w_im=w_im.reshape(B, dg * kk, Ho, Wo))


def dcn_pin_groups():
    """Every DCN input of the reference pin, by group: all inputs of the GPU suite's DCN tests, the lattice and the pin's own fuzz."""
    return {
        "kernel": [dcn_kernel_case(*row, sig=sig) for row in DCN_KERNEL_SHAPES for sig in (False, True)],
        "split_k": [dcn_splitk_case(*row, sig=sig) for row in DCN_SPLITK_SHAPES for sig in (False, True)],
        "kernel_dg": [dcn_kernel_dg_case(*row) for row in DCN_KERNEL_DG_SHAPES],
        "forward_dg": [dcn_forward_dg_case(*row) for row in DCN_FORWARD_DG_ROWS],
        "full_args": [dcn_full_arg_case(*row) for row in DCN_FULL_ARG_ROWS],
        "gpu_fuzz": dcn_gpu_fuzz_cases(),
        "lattice": [dcn_lattice_case(*row) for row in DCN_LATTICE_CONFIGS],
        "pin_fuzz": dcn_pin_fuzz_cases(),
    }


# one kernel shape per tile code also in the logits mode (the smallest of each)
DCN_FIXTURE_LOGITS_SHAPES = [(256, 64, 5, 6, True, 0), (16, 64, 9, 7, True, 64064), (48, 128, 6, 10, True, 64128), (32, 64, 12, 12, True, 128064),
                             (32, 32, 9, 13, True, 128032), (48, 64, 5, 9, True, 64032)]


def dcn_fixtures():
    """name -> (zero-argument generator of the case) for every committed reference output tests/golden/dcn_ref_<name>.npz.  The
    files hold the float32-rounded output of the reference forward (oracle.dcn.dcn_v2_forward_ref) only; inputs come from here."""
    fx = {}
    for row in DCN_KERNEL_SHAPES:
        fx["kernel_%d_%d_%dx%d_mask" % row[:4]] = (lambda row=row: dcn_kernel_case(*row, sig=False))
    for row in DCN_FIXTURE_LOGITS_SHAPES:
        assert row in DCN_KERNEL_SHAPES
        fx["kernel_%d_%d_%dx%d_logits" % row[:4]] = (lambda row=row: dcn_kernel_case(*row, sig=True))
    for row in DCN_SPLITK_SHAPES:
        fx["splitk_%d_%d_%dx%d_s%d" % row[:5]] = (lambda row=row: dcn_splitk_case(*row, sig=False))
    for row in DCN_KERNEL_DG_SHAPES:
        fx["kerneldg_%d_%d_g%d_s%d" % (row[0], row[1], row[2], row[4])] = (lambda row=row: dcn_kernel_dg_case(*row))
    for row in DCN_FULL_ARG_ROWS:
        fx["fullargs_" + "_".join(str(v) for v in row)] = (lambda row=row: dcn_full_arg_case(*row))
    for row in DCN_LATTICE_CONFIGS:
        fx["lattice_" + row[0]] = (lambda row=row: dcn_lattice_case(*row))
    return fx


# ---------------------------------------------------------------------------------------------------------------------
# Decode decisions at their limits (tests/test_decode_edges_*.py, tests/golden/make_golden.py decode_edges).
#
# Every scene is built from dyadic values, so that the arithmetic of the reference's multi_pose_decode (decode.py:244-304) is exact
# and the side of each comparison is known by construction (and asserted here).  A TRIPLET is one scene three times: the moving
# operand one float32 below its limit (side -1), exactly on it (0) and one float32 above (+1).  The comparisons:
ASSIGN_COMPARISONS = ("sx<l", "sx>r", "sy<t", "sy>b", "ss<0.1", "best>lim", "s>0.1")


def _next(v, up):
    return F32(np.nextafter(F32(v), F32(np.inf if up else -np.inf)))


def _around(v):
    """side -> the float32 below / on / above v."""
    return {-1: _next(v, False), 0: F32(v), 1: _next(v, True)}


def _exact_sum(a, b):
    """float32(a) + float32(b) in float32, asserted exact."""
    s = F32(a) + F32(b)
    assert float(s) == float(F32(a)) + float(F32(b)), (a, b)
    return s


def _fillers(H, W, n):
    pos = [(y, x) for y in (H - 2, 2) for x in range(W - 2, 0, -4)]
    assert len(pos) >= n
    return pos[:n]


def edge_scene(H=16, W=16, K=4, centre=(8, 8), wh=(8.0, 8.0), reg=(0.0, 0.0), joints=()):
    """One image.  Centre plane: the main centre (score 0.5, rank 0) and K + 2 lower, distinct fillers far from it, so that the
    top-(K+1) of the plane has no tie.  joints: per joint (hps_x, hps_y, [(y, x, score, off_x, off_y), ...]) -- hps / wh / reg are
    constant maps, hp_offset is zero but at the candidates; each joint plane gets K + 2 distinct fillers of at most 1/16 (under the
    0.1 threshold: -1 / -10000 sentinels)."""
    J = len(joints)
    hm = np.zeros((1, 1, H, W), F32)
    hm_hp = np.zeros((1, J, H, W), F32)
    hps = np.zeros((1, 2 * J, H, W), F32)
    off = np.zeros((1, 2, H, W), F32)
    hm[0, 0, centre[0], centre[1]] = 0.5
    fill = _fillers(H, W, K + 2)
    for i, (y, x) in enumerate(fill):
        assert abs(y - centre[0]) > 1
        hm[0, 0, y, x] = (16 - i) / 64.0
    for j, (hx, hy, cands) in enumerate(joints):
        hps[0, 2 * j], hps[0, 2 * j + 1] = hx, hy
        for i, (y, x) in enumerate(fill):
            hm_hp[0, j, y, x] = (16 - i) / 256.0
        for (y, x, s, ox, oy) in cands:
            assert min(abs(y - fy) for fy, _ in fill) > 1 and hm_hp[0, j, y, x] == 0
            hm_hp[0, j, y, x] = s
            assert (off[0, :, y, x] == 0).all() or (off[0, 0, y, x] == F32(ox) and off[0, 1, y, x] == F32(oy))
            off[0, 0, y, x], off[0, 1, y, x] = ox, oy
    whm = np.empty((1, 2, H, W), F32)
    whm[0, 0], whm[0, 1] = wh
    regm = np.empty((1, 2, H, W), F32)
    regm[0, 0], regm[0, 1] = reg
    return dict(hm=hm, wh=whm, hps=hps, reg=regm, hm_hp=hm_hp, hp_offset=off)


def _stack(*scenes):
    return {k: np.concatenate([s[k] for s in scenes], 0) for k in scenes[0]}


def _plain_joint(c=(8, 8)):
    """A joint with one accepted candidate on the centre, far from every limit."""
    return (0.25, 0.25, [(c[0], c[1], 0.75, 0.5, 0.5)])


def decode_assign_edges():
    """name -> dict(inp, K, use_reg, use_off, group, side, cmp, j).  group / side / cmp are None for the cases that are no triplet
    member; the decision under test is the one of image 0, centre rank 0 (the 0.5 peak), joint j."""
    out = {}

    def add(name, inp, K=4, use_reg=True, use_off=True, group=None, side=None, cmp=None, j=0):
        assert name not in out
        out[name] = dict(inp=inp, K=K, use_reg=use_reg, use_off=use_off, group=group, side=side, cmp=cmp, j=j)

    names = {-1: "below", 0: "at", 1: "above"}
    # -- box edges: centre (8, 8), wh 8, reg 0 -> l = t = 4, r = b = 12; the candidate sits on the edge pixel and hp_offset moves it
    edges = {"left": ("sx<l", 8, 4, 0, -3.75, 0.25), "right": ("sx>r", 8, 12, 0, 3.75, 0.25),
             "top": ("sy<t", 4, 8, 1, 0.25, -3.75), "bottom": ("sy>b", 12, 8, 1, 0.25, 3.75)}
    for ename, (cmp, y, x, axis, hx, hy) in edges.items():
        base = (x, y)[axis]
        for side, target in _around(base).items():
            o = F32(float(target) - base)
            assert _exact_sum(base, o) == target
            cand = (y, x, 0.75, o if axis == 0 else 0.0, o if axis == 1 else 0.0)
            if axis == 0:
                add("%s_%s" % (ename, names[side]), edge_scene(joints=[(hx, hy, [cand])]), group=ename, side=side, cmp=cmp)
            else:                           # two joints, the decision in the second
                add("%s_%s" % (ename, names[side]), edge_scene(joints=[_plain_joint(), (hx, hy, [cand])]), group=ename, side=side,
                    cmp=cmp, j=1)
    # the right-edge triplet again as image 0 of a batch of two 32 x 32 maps with K = 8 (image 1: the top edge, exactly on it)
    for side, target in _around(12).items():
        o = F32(float(target) - 12)
        im0 = edge_scene(32, 32, 8, joints=[(3.75, 0.25, [(8, 12, 0.75, o, 0.0)]), _plain_joint()])
        im1 = edge_scene(32, 32, 8, joints=[_plain_joint(), (0.25, -3.75, [(4, 8, 0.75, 0.0, 0.0)])])
        add("b2_right_%s" % names[side], _stack(im0, im1), K=8, group="b2_right", side=side, cmp="sx>r")
    # -- candidate score on 0.1: the joint plane's peak (fillers <= 1/16).  Under and on 0.1 it is masked to the sentinels, and then
    # no candidate of the plane is valid: ss = -1.  (`ss < 0.1f` never sees equal operands: ss is -1 or a score above 0.1.)
    for side, s in _around(0.1).items():
        add("score_%s" % names[side], edge_scene(joints=[(0.25, 0.25, [(8, 8, s, 0.0, 0.0)])]), group="score", side=side, cmp="s>0.1")
    # the same with a second, valid candidate outside the distance limit: ss is then a score, never -1
    for side, s in _around(0.1).items():
        add("score2_%s" % names[side], edge_scene(joints=[(0.25, 0.25, [(8, 8, s, 0.0, 0.0), (8, 11, 0.5, 0.0, 0.0)])]),
            group="score2", side=side, cmp="s>0.1")
    # -- distance limit fl(8 * 0.3f): candidate at x = 1 (sx = 1), centre at x = 2, dy = 0, kx = 1 + d with d below / on / above the
    # limit; once max(h, w) = h and once = w.  Three joints, the decision in the last.
    lim = F32(F32(8) * F32(0.3))
    for tag, whv in (("h", (4.0, 8.0)), ("w", (8.0, 4.0))):
        for side, d in _around(lim).items():
            kx = _exact_sum(1, d)
            hx = F32(float(kx) - 2)
            assert _exact_sum(hx, 2) == kx and F32(kx - F32(1)) == d
            assert np.sqrt(F32(d * d) + F32(0) * F32(0), dtype=F32) == d      # the float32 distance IS d
            sc = edge_scene(centre=(8, 2), wh=whv, joints=[_plain_joint((8, 2)), _plain_joint((8, 2)), (hx, 0.0, [(8, 1, 0.75, 0.0, 0.0)])])
            add("dist_%s_%s" % (tag, names[side]), sc, group="dist_" + tag, side=side, cmp="best>lim", j=2)
    # -- equal distances: candidates symmetric about the regressed point (8, 8); the first in the joint's top-K order wins
    add("tie_left_first", edge_scene(joints=[(0.0, 0.0, [(8, 6, 0.75, 0.0, 0.0), (8, 10, 0.5, 0.0, 0.0)])]))
    add("tie_right_first", edge_scene(joints=[(0.0, 0.0, [(8, 6, 0.5, 0.0, 0.0), (8, 10, 0.75, 0.0, 0.0)])]))
    add("tie_three", edge_scene(joints=[(0.0, 0.0, [(8, 6, 0.5, 0.0, 0.0), (8, 10, 0.75, 0.0, 0.0), (6, 8, 0.625, 0.0, 0.0)])]))
    # -- a joint plane without any candidate above 0.1: K equal distances to (-10000, -10000), index 0 wins, score -1
    add("no_candidate", edge_scene(joints=[_plain_joint(), (0.25, 0.25, [])]), j=1)
    # -- the +0.5f branches.  reg=None: cx = 8.5, l = 4.5, hp_offset moves the candidate of pixel x = 4 through it
    for side, target in _around(4.5).items():
        o = F32(float(target) - 4)
        assert _exact_sum(4, o) == target
        add("noreg_left_%s" % names[side], edge_scene(joints=[(-3.25, 0.25, [(8, 4, 0.75, o, 0.0)])]), use_reg=False,
            group="noreg_left", side=side, cmp="sx<l")
    # reg=None and hp_offset=None: sx = 4.5 stays, wh moves l = 8.5 - w / 2 through it (side: sx relative to l)
    for side, lt in ((-1, _next(4.5, True)), (0, F32(4.5)), (1, _next(4.5, False))):
        w = F32(2 * (8.5 - float(lt)))
        assert F32(F32(8.5) - w / F32(2)) == lt and float(w) == 2 * (8.5 - float(lt))
        add("nooff_left_%s" % names[side], edge_scene(wh=(w, 8.0), joints=[(-3.25, 0.75, [(8, 4, 0.75, 0.0, 0.0)])]), use_reg=False,
            use_off=False, group="nooff_left", side=side, cmp="sx<l")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# More than one centre class.  name -> (cat, H, W, K, J, seed, seam)
DECODE_MULTICAT_CASES = {
    "cat4_64x64": (4, 64, 64, 100, 2, 501, False),         # 16 384 keys: register path, power-of-two index math across planes
    "cat3_32x48": (3, 32, 48, 40, 2, 502, False),          # register path, division index math
    "cat2_15x17": (2, 15, 17, 9, 2, 503, False),           # planes not 16-byte aligned
    "cat2_128x96": (2, 128, 96, 100, 2, 504, False),       # 24 576 keys: LDS path without registers
    "cat3_128x128": (3, 128, 128, 100, 2, 505, False),     # 49 152 keys: 2 chunks of 24 576, the first ends inside plane 1
    "cat5_100x131": (5, 100, 131, 256, 2, 506, False),     # 65 500 keys: 2 odd chunks, neither boundary on a map row
    "seam_cat4_64x64": (4, 64, 64, 100, 1, 511, True),
    "seam_cat2_15x17": (2, 15, 17, 9, 1, 512, True),
    "seam_cat2_128x96": (2, 128, 96, 100, 1, 513, True),
    "seam_cat3_128x128": (3, 128, 128, 100, 1, 514, True),
}


def seam_peaks(cat, H, W):
    """(class, y, x, value) of the peaks the seam cases plant beside a plane boundary; NMS has to keep every one."""
    out = []
    for c in range(cat - 1):
        out.append((c, H - 1, 5, 2.0 + c / 16.0))            # last row of plane c; larger values follow it in memory
        out.append((c + 1, 0, W - 6, 2.5 + c / 16.0))        # row 0 of plane c + 1; larger values precede it in memory
    return out


def decode_multicat(cat, H, W, J, seed, seam=False):
    r = np.random.RandomState(seed)
    inp = decode_random(seed, B=1, H=H, W=W, J=J)
    hm = sigmoid(r.randn(1, cat, H, W))
    if seam:
        for c in range(cat - 1):
            hm[0, c + 1, 0, 4:7] = np.array([3.0, 3.25, 3.5]) + c / 16.0       # "below" the peak (H-1, 5) of plane c
            hm[0, c, H - 1, W - 7:W - 4] = np.array([4.0, 4.25, 4.5]) + c / 16.0   # "above" the peak (0, W-6) of plane c + 1
        for (c, y, x, v) in seam_peaks(cat, H, W):
            hm[0, c, y, x] = v
    inp["hm"] = hm
    return inp


# ---------------------------------------------------------------------------------------------------------------------
# Zeros inside the top-K, quantised ties, signed maps (the oracle's order rule is the reference: value desc, flat index asc)
def decode_sparse(seed, H, W, J=2):
    """Every plane: 20..60 planted, distinct positive values, zeros everywhere else."""
    r = np.random.RandomState(seed)
    inp = decode_random(seed, B=1, H=H, W=W, J=J)
    for key in ("hm", "hm_hp"):
        m = np.zeros_like(inp[key])
        for plane in m.reshape(-1, H * W):
            n = r.randint(20, 61)
            plane[r.choice(H * W, n, replace=False)] = ((r.permutation(4096)[:n] + 1) / 4096.0).astype(F32)
        inp[key] = m
    return inp


def decode_quantised(seed, H, W, J=2):
    inp = decode_random(seed, B=1, H=H, W=W, J=J)
    for key in ("hm", "hm_hp"):
        inp[key] = (np.round(inp[key] * 16) / 16).astype(F32)
    return inp


def decode_signed(seed, H, W, J=2, zeros=0):
    """hm / hm_hp straight from randn (no sigmoid).  zeros > 0: that many true zeros planted per plane, and two 5 x 5 patches made
    negative throughout (below -1, their centres -0.25 and -0.5), so that the plane has negative PEAKS (the maximum of nine normal
    values is hardly ever negative)."""
    r = np.random.RandomState(seed)
    inp = decode_random(seed, B=1, H=H, W=W, J=J)
    for key in ("hm", "hm_hp"):
        m = r.randn(*inp[key].shape).astype(F32)
        for plane in m.reshape(-1, H, W):
            if zeros:
                plane.reshape(-1)[r.choice(H * W, zeros, replace=False)] = 0.0
                for y0, peak in ((1, -0.25), (H - 6, -0.5)):
                    plane[y0:y0 + 5, y0:y0 + 5] = -np.abs(plane[y0:y0 + 5, y0:y0 + 5]) - F32(1)
                    plane[y0 + 2, y0 + 2] = peak
        inp[key] = m
    return inp


# name -> (seed, H, W, K): K small enough that only positive peaks are selected (asserted from the oracle where it is used)
DECODE_SIGNED_CASES = {"signed_16x16": (601, 16, 16, 5), "signed_60x70": (602, 60, 70, 40), "signed_128x129": (603, 128, 129, 100)}
