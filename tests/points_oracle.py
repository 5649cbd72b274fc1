"""TEST INFRASTRUCTURE ONLY -- the detections-only head kernels of csrc/head_points.hip, per element against float64.

`head_points_kernel<1>` / `<2>` (cp_head_points_f32) and `head_points_pairs_kernel<1>` / `<2>` (cp_head_points_pairs_f32) evaluate the
wh / hps / reg branches of the keypoint head at the decoded centre peaks and hp_offset at the joint peaks.  tests/test_head_points_hip.py
and tests/test_flip_dets_only_hip.py hold them to `max|got - ref| <= 1e-4 max|ref|` over a whole map at one geometry on dense features.
This module is the table of launches (`ROWS` -> `CASES`), the case builder (`make_case`), the reference (`reference`), the judging
(`judge_flat`), a numpy emulation of the kernels' data path with the mutations a wrong kernel would show (`emulate`) and the device run
(`run_case`, `run_plan_case`), on top of `layer_oracle` (`head_branch`, `c_for`, `spread_factors`, `worst_ratio`).

* Reference: every branch is `layer_oracle.head_branch` -- dense 3x3 + bias + ReLU -> 1x1 + bias in float64 with its magnitude sum A and
  term count K -- read at the addressed pixels.  Under the flip test the merged value is (a + sign t) / 2 with a from image 2n at (y, x)
  and t from image 2n + 1 at (y, W-1-x), channel 2 perm[c >> 1] + (c & 1), sign = -1 for the even channels of hps; reg and hp_offset are
  the image's own.  The merged A is (A_a + A_t) / 2 and K grows by 2 (the merge's two roundings).
* Bound: |out - ref64| <= c_for("direct", K) u A at every addressed element.  No constant here comes from device output.
* Inputs: post-ReLU features (about half zeros) with `spread_factors` on the channels, on the rows of every 3x3 weight (and its bias) and
  on the rows of every 1x1 weight (and its bias).  `feat` is a channel slice, FEAT_OFF floats into the pixels of a NaN-filled buffer that
  is FEAT_PAD floats wider, with one NaN image before and after; `out` is NaN-filled with G guard floats on both sides.
* Point lists are built per row (`point_list`), not drawn: corners, edge midpoints, a duplicated centre, one pixel addressed by three
  joints, a joint index equal to a centre index, one negative index and one index in class plane 3, as many of them as K and J leave
  room for (`SPECIALS` in the order they are kept).

The index rule is stated once: `pixel`.  `geometry` restates the launchers' block and grid arithmetic; tests/test_points_oracle_cpu.py
holds every row's claim against it.
"""
import collections
import functools
import time

import numpy as np
import torch
import torch.nn.functional as F

import layer_oracle as lo

SPARSE = ("wh", "hps", "reg", "hp_offset")
HP_M = 32                                                  # points per block
G = 64                                                     # guard floats on both sides of `out`
FEAT_OFF, FEAT_PAD = 4, 12                                 # the slice starts 16 bytes into a pixel; featLd = C + FEAT_PAD
MAX_THREADS, MAX_LDS = 512, 160 * 1024                     # __launch_bounds__ of the kernels; LDS of one gfx950 workgroup
LDS_RESERVE = 64 * 1024                                    # above this a kernel needs its dynamic LDS limit raised
MUST_COVER = ("head_points_kernel<1>", "head_points_kernel<2>", "head_points_pairs_kernel<1>", "head_points_pairs_kernel<2>")
REFUSED_HC = (288, 352, 416, 480)
SERVED_HC = (256, 320, 448, 512)
# liveness floors on the test's own data: the share of hidden pre-activations the ReLU zeroes lies strictly inside RELU_SHARE, and
# more than HPS_LIVE[1] of the addressed hps elements are at least HPS_LIVE[0] times their own bound c u A in magnitude (an element no
# larger than its tolerance checks no sign and no permutation: a merge that cancelled everything would pass whatever it did)
RELU_SHARE = (0.1, 0.9)
HPS_LIVE = (100.0, 0.5)

f32, f64 = torch.float32, torch.float64


def pixel(ind, HW):
    """the pixel a decoded index addresses: the class plane dropped, a negative index wrapped"""
    return ((ind % HW) + HW) % HW


def nout(name, J):
    return 2 * J if name == "hps" else 2


def default_perm(J):
    """the joint permutation of the flip test: COCO's left / right pairs for J = 17, neighbours swapped otherwise (an involution)"""
    perm = list(range(J))
    for a in range(1, J - 1, 2):
        perm[a], perm[a + 1] = a + 1, a
    return tuple(perm)


# ---- the table --------------------------------------------------------------------------------------------------------------------------
# B: images (cp_head_points_f32) resp. image / twin pairs (cp_head_points_pairs_f32).  entries: which entry points run the row.
# claim: what the row is there to reach, asserted against `geometry` (and `point_list`) in tests/test_points_oracle_cpu.py.
Row = collections.namedtuple("Row", "id regimes B H W C hc J K perm entries claim")
BOTH = ("points", "pairs")


def _r(id, regimes, B=2, H=5, W=7, C=16, hc=32, J=3, K=12, perm=None, entries=BOTH, **claim):
    return Row(id, tuple(regimes.split()), B, H, W, C, hc, J, K, tuple(perm) if perm else default_perm(J), entries, claim)


ROWS = [
    _r("w1-c16-hc32", "W1", ns=1, nthr=64, kgroups=2),
    _r("odd-c48-hc96", "ODD", C=48, hc=96, ns=1, nthr=192),
    _r("odd-hc320", "ODD", hc=320, ns=2, nthr=320),
    _r("odd-hc448", "ODD", hc=448, ns=2, nthr=448),
    _r("wide-hc224", "WIDE", hc=224, ns=1, nthr=448),                       # the widest block of <1>
    _r("wide-c64-hc256", "WIDE", C=64, hc=256, ns=2, nthr=256),
    _r("wide-c64-hc128", "WIDE", C=64, hc=128, ns=2, nthr=128),
    _r("lds-c512-hc512", "LDS J", B=2, H=7, W=9, C=512, hc=512, J=17, K=8, ns=2, nthr=512, lds=131712, lds_pairs=136064),
    _r("one-1x1", "ONE", B=1, H=1, W=1, J=1, K=1, ctiles=1, jtiles=1, last_c=1, last_j=1),
    _r("one-1x5", "ONE", B=1, H=1, W=5, J=1, K=1, ctiles=1, jtiles=1, last_c=1, last_j=1),
    _r("one-5x1", "ONE", B=1, H=5, W=1, J=1, K=1, ctiles=1, jtiles=1, last_c=1, last_j=1),
    _r("tile-32", "TILE", B=2, K=16, ctiles=1, last_c=32, jtiles=3, last_j=32),
    _r("tile-33", "TILE", B=3, K=11, ctiles=2, last_c=1, jtiles=4, last_j=3),
    _r("k256", "K256", B=1, H=16, W=17, J=2, K=256, ctiles=8, jtiles=16),
    _r("j1", "J", J=1),
    _r("j17", "J", J=17),
    _r("mirror-w7", "MIRROR", H=4, W=7, hc=64, J=17, entries=("pairs",), ns=1, nthr=128),
    _r("mirror-3cyc", "MIRROR-3CYC J", H=4, W=6, J=4, perm=(1, 2, 0, 3), entries=("pairs",)),
]
ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)
CASES = ["%s/%s" % (r.id, e) for r in ROWS for e in r.entries]
REGIMES = ("W1", "ODD", "WIDE", "LDS", "ONE", "TILE", "K256", "J", "MIRROR", "MIRROR-3CYC")


def geometry(row, pairs):
    """the launchers' arithmetic restated: dict(ns, nthr, lds, ctiles, jtiles, last_c, last_j, grid, kernel, kgroups)"""
    ns = 2 if row.hc % 64 == 0 and row.hc >= 128 else 1
    nthr = 64 * row.hc // (32 * ns)
    lds = HP_M * (row.C + 4) * 4 + HP_M * (row.hc + 1) * 4 + (HP_M * 2 * row.J * 4 if pairs else 0)
    nc, nj = row.B * row.K, row.B * row.J * row.K
    ctiles, jtiles = -(-nc // HP_M), -(-nj // HP_M)
    return dict(ns=ns, nthr=nthr, lds=lds, ctiles=ctiles, jtiles=jtiles, last_c=nc - HP_M * (ctiles - 1), last_j=nj - HP_M * (jtiles - 1),
                grid=3 * ctiles + jtiles, kgroups=row.C // 8,
                kernel=("head_points_pairs_kernel<%d>" if pairs else "head_points_kernel<%d>") % ns)


def accepted(row):
    """the launchers' argument checks on the row's shape (csrc/head_points.hip)"""
    g = geometry(row, True)
    return (row.B > 0 and row.H > 0 and row.W > 0 and row.J > 0 and 0 < row.K <= min(256, row.H * row.W) and row.C % 16 == 0 and
            0 < row.C <= 512 and row.hc % 32 == 0 and 0 < row.hc <= 512 and g["nthr"] <= MAX_THREADS and g["lds"] <= MAX_LDS)


# ---- point lists ------------------------------------------------------------------------------------------------------------------------
SPECIALS = ("corner00", "corner11", "negative", "plane3", "dup", "dup2", "corner01", "corner10", "left", "right", "top", "bottom")


def special_index(name, H, W):
    """the flat index of one special centre (`dup2` repeats `dup`: the interior pixel next to the centre of the map)"""
    HW = H * W
    return {"corner00": 0, "corner01": W - 1, "corner10": (H - 1) * W, "corner11": HW - 1, "left": (H // 2) * W, "right": (H // 2) * W + W - 1,
            "top": W // 2, "bottom": (H - 1) * W + W // 2, "dup": (H // 2) * W + W // 2, "dup2": (H // 2) * W + W // 2,
            "negative": -(HW // 3) - 1, "plane3": 3 * HW + (HW * 2) // 5 + 1}[name]


def point_list(row, seed=0):
    """-> (inds int32 [B, 1+J, K], {special: (b, list row, k)} of image 0).  Centre rows: the first K of SPECIALS, then random pixels.
    Joint rows: the last one holds the corners and edge midpoints in reverse order; joints 1, 2 and 3 share one pixel in one column;
    joint 1 addresses the pixel of the centre list's second entry (corner11).  K = 1 keeps one special, chosen per row id."""
    r = np.random.RandomState(1000 + seed)
    B, H, W, J, K = row.B, row.H, row.W, row.J, row.K
    HW = H * W
    inds = r.randint(0, HW, size=(B, 1 + J, K)).astype(np.int64)
    names = list(SPECIALS[:K])
    if K == 1:
        names = [{"one-1x1": "negative", "one-1x5": "plane3"}.get(row.id, "dup")]
    where = {}
    for b in range(B):
        for k, name in enumerate(names):
            inds[b, 0, k] = special_index(name, H, W)
            if b == 0:
                where[name] = (0, 0, k)
        edge = [special_index(n, H, W) for n in ("corner00", "corner01", "corner10", "corner11", "left", "right", "top", "bottom")][::-1]
        n = min(K, len(edge))
        inds[b, J, :n] = edge[:n]
        k3 = K - 1 if K > len(edge) else 1                                  # (clear of the edge list when the last joint is joint 3)
        if J >= 3 and K >= 2:
            inds[b, 1, k3] = inds[b, 2, k3] = inds[b, 3, k3] = special_index("dup", H, W) - (1 if W > 1 else 0)
            if b == 0:
                where["three_joints"] = (0, 1, k3)
        kj = 0 if J > 1 else K - 1
        if (K >= 2 or J >= 2) and (J > 1 or K > len(edge)):
            inds[b, 1, kj] = pixel(int(inds[b, 0, min(1, K - 1)]), HW)
            if b == 0:
                where["joint_is_centre"] = (0, 1, kj)
    return torch.from_numpy(inds.astype(np.int32)), where


def shuffled(inds, HW, seed=11):
    """every list row of `inds` permuted and padded with duplicates of its own entries, as far as K <= 256 and K <= H W leave room:
    the same set of addressed pixels -> (inds2, K2)"""
    B, R, K = inds.shape
    K2 = K + max(0, min(9, 256 - K, HW - K))
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(B, R, K2, dtype=torch.int32)
    for b in range(B):
        for j in range(R):
            order = torch.randperm(K, generator=g)
            extra = torch.randint(0, K, (K2 - K,), generator=g)
            out[b, j] = torch.cat([inds[b, j][order], inds[b, j][extra]])
    return out, K2


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one launch: the row, its entry point, the logical data (x NCHW float32, sd) and the physical buffers (featbuf, inds)"""

    def __init__(self, row, pairs, x, sd, inds, where):
        self.row, self.pairs, self.x, self.sd, self.inds, self.where = row, pairs, x, sd, inds, where
        self.nimg = x.shape[0]
        self.ld = row.C + FEAT_PAD
        self.featbuf = torch.full((self.nimg + 2, row.H, row.W, self.ld), float("nan"))
        self.featbuf[1:-1, :, :, FEAT_OFF:FEAT_OFF + row.C] = x.permute(0, 2, 3, 1)
        self.geo = geometry(row, pairs)

    @property
    def feat(self):
        return self.featbuf[1:-1, :, :, FEAT_OFF:FEAT_OFF + self.row.C]

    @property
    def out_floats(self):
        return self.row.B * self.row.H * self.row.W * (6 + 2 * self.row.J)


def branch_weights(C, hc, J, g):
    """the four branches under layer_oracle's key names ("wh.0.weight", "wh.2.bias", ...), `spread_factors` on the rows"""
    sd = {}
    for name in SPARSE:
        n = nout(name, J)
        fh, fn = lo.spread_factors(hc), lo.spread_factors(n)
        sd[name + ".0.weight"] = torch.randn(hc, C, 3, 3, generator=g) / (3.0 * C ** 0.5) * fh.view(-1, 1, 1, 1)
        sd[name + ".0.bias"] = torch.randn(hc, generator=g) * 0.1 * fh
        sd[name + ".2.weight"] = torch.randn(n, hc, 1, 1, generator=g) / hc ** 0.5 * fn.view(-1, 1, 1, 1)
        sd[name + ".2.bias"] = torch.randn(n, generator=g) * 0.1 * fn
    return sd


@functools.lru_cache(maxsize=None)
def make_case(cid):
    rid, entry = cid.split("/")
    row, pairs = ROW[rid], entry == "pairs"
    seed = 2 * ROWS.index(row) + pairs
    g = torch.Generator().manual_seed(4000 + seed)
    nimg = row.B * (2 if pairs else 1)
    x = torch.relu(torch.randn(nimg, row.C, row.H, row.W, generator=g)) * lo.spread_factors(row.C).view(1, -1, 1, 1)
    inds, where = point_list(row, seed)
    return Case(row, pairs, x, branch_weights(row.C, row.hc, row.J, g), inds, where)


# ---- reference --------------------------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "val A K")


def merge_maps(val, row, name, sign_first=True):
    """the flip test's merge of the [2N] maps `val` of branch `name` in val.dtype -> [N]; hps: twin channel 2 perm[c >> 1] + (c & 1) with
    sign -1 on the even channels; wh: the mirrored twin; reg / hp_offset: the image's own"""
    a, t = val[0::2], torch.flip(val[1::2], [3])
    if name in ("reg", "hp_offset"):
        return a
    two = torch.tensor(2.0, dtype=val.dtype)
    if name == "wh":
        return (a + t) / two
    cs = [2 * row.perm[c >> 1] + (c & 1) for c in range(2 * row.J)]
    sign = torch.tensor([-1.0 if c % 2 == 0 else 1.0 for c in range(2 * row.J)], dtype=val.dtype).view(1, -1, 1, 1)
    return (a + t[:, cs] * sign) / two


def merge_A(A, row, name):
    a, t = A[0::2], torch.flip(A[1::2], [3])
    if name in ("reg", "hp_offset"):
        return a
    if name == "hps":
        t = t[:, [2 * row.perm[c >> 1] + (c & 1) for c in range(2 * row.J)]]
    return (a + t) / 2


def evaluate(row, pairs, x, sd, dt):
    """{name: Ref} of the dense maps ([B, n, H, W], merged under `pairs`) from the logical features x [images, C, H, W] in `dt`"""
    out = {}
    xv = x.to(dt)
    with torch.no_grad():
        for name in SPARSE:
            o = lo.head_branch(sd, xv, name + ".0", name + ".2", row.hc, nout(name, row.J), None, dt)
            val, A, K = o.val, o.A, o.K
            if pairs:
                val = merge_maps(val, row, name)
                A = None if A is None else merge_A(A, row, name)
                K += 2
            out[name] = Ref(val, A, K)
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    c = make_case(cid)
    return evaluate(c.row, c.pairs, c.x, c.sd, f64)


def addressed(row, inds, name):
    """bool [B, 1, H, W]: the pixels the launch writes in the maps of branch `name`"""
    HW = row.H * row.W
    mask = torch.zeros(row.B, HW, dtype=torch.bool)
    for b in range(row.B):
        idx = inds[b, 1:].reshape(-1) if name == "hp_offset" else inds[b, 0]
        mask[b, pixel(idx.long(), HW)] = True
    return mask.view(row.B, 1, row.H, row.W)


def relu_zero_share(case):
    """share of the hidden pre-activations (all four branches, every pixel, float32) that the ReLU zeroes"""
    zero = total = 0
    for name in SPARSE:
        pre = F.conv2d(case.x, case.sd[name + ".0.weight"], case.sd[name + ".0.bias"], padding=1)
        zero, total = zero + int((pre <= 0).sum()), total + pre.numel()
    return zero / total


# ---- judging ----------------------------------------------------------------------------------------------------------------------------
def split_flat(flat, row):
    """the flat output (guards included) -> ({name: [B, n, H, W]}, front guard, back guard)"""
    maps, off = {}, G
    for name in SPARSE:
        n = row.B * nout(name, row.J) * row.H * row.W
        maps[name] = flat[off:off + n].view(row.B, nout(name, row.J), row.H, row.W)
        off += n
    assert off + G == flat.numel()
    return maps, flat[:G], flat[off:]


def judge_flat(row, inds, ref, flat):
    """flat float32 CPU output against {name: Ref} -> dict(worst {name: Worst}, c, failures [text], bad {(name, b, n, y, x)}):
    the bound at every addressed element, NaN at every other one, NaN guards"""
    maps, g0, g1 = split_flat(flat, row)
    rep = dict(worst={}, failures=[], bad=set(), c=0.0)
    if not (bool(torch.isnan(g0).all()) and bool(torch.isnan(g1).all())):
        rep["failures"].append("guard floats written")
    for name in SPARSE:
        got, r = maps[name], ref[name]
        mask = addressed(row, inds, name).expand_as(got)
        stray = ~mask & ~torch.isnan(got)
        for loc in stray.nonzero().tolist()[:8]:
            rep["failures"].append("%s: element %s is not addressed and not NaN" % (name, tuple(loc)))
        c = lo.c_for("direct", r.K)
        rep["c"] = max(rep["c"], c)
        err = (got.double() - r.val).abs()
        err = (err - lo.FLT_MIN).clamp_(min=0.0)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / (lo.U * r.A))
        ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
        i = int(torch.argmax(ratio))
        loc = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        rep["worst"][name] = lo.Worst(float(ratio.reshape(-1)[i]), loc, float(err.reshape(-1)[i]), float(r.A.reshape(-1)[i]))
        over = ratio > c
        rep["bad"].update((name,) + tuple(l) for l in over.nonzero().tolist())
        rep["bad"].update((name,) + tuple(l) for l in stray.nonzero().tolist())
        if bool(over.any()):
            w = rep["worst"][name]
            rep["failures"].append("%s: %d elements over the bound, worst err %.3e = %.1f u A (A = %.3e) > c = %.1f at (b, c, y, x) = %s"
                                   % (name, int(over.sum()), w.err, w.ratio, w.A, c, w.loc))
    return rep


def worst_of(rep):
    return max(rep["worst"].values(), key=lambda w: w.ratio)


def hps_liveness(row, inds, ref):
    """share of the addressed hps elements with |ref| > HPS_LIVE[0] c u A"""
    r = ref["hps"]
    mask = addressed(row, inds, "hps").expand_as(r.val)
    return float((r.val.abs() > HPS_LIVE[0] * lo.c_for("direct", r.K) * lo.U * r.A)[mask].double().mean())


# ---- numpy emulation of the kernels' data path -----------------------------------------------------------------------------------------
# Point table in block order, per-tap gather from the PHYSICAL feature buffer (pointer, featLd) with zero padding, the taps accumulated in
# order in float32 (one matrix product per tap), bias + ReLU, the 1x1 as a sequential float32 sum over the hidden channels, the image
# side parked, the twin side merged, the scatter into the flat NCHW maps.  A mutation (kind, b, p) changes the path of the points of
# image / pair b at pixel p alone, so the mutated elements are the outputs at (b, p):
MUTATIONS = ("wrap_border", "next_image", "no_modulo", "ld_is_C", "no_relu", "drop_hidden")
MUTATIONS_PAIRS = ("twin_at_x", "sign_on_odd", "no_perm", "perm_inverted", "parked_neighbour")


def lowest_spread_row(n):
    return int(lo.spread_factors(n).argmin())


def _one_by_one(hid, w2, skip=None):
    """sequential float32 sum over the hidden channels: hid [P, hc], w2 [n, hc] -> [P, n]; skip: (point, output, hidden channel) left out"""
    v = np.zeros((hid.shape[0], w2.shape[0]), np.float32)
    for c in range(hid.shape[1]):
        t = (hid[:, c:c + 1] * w2[None, :, c]).astype(np.float32)
        if skip is not None and c == skip[2]:
            t[skip[0], skip[1]] = 0.0
        v = (v + t).astype(np.float32)
    return v


def emulate(case, mut=None, inds=None):
    """-> the flat float32 output (torch, guards included) the kernels' data path gives for `case` (with `inds` instead of its own)"""
    row, pairs = case.row, case.pairs
    B, H, W, C, hc, J = row.B, row.H, row.W, row.C, row.hc, row.J
    inds = (case.inds if inds is None else inds).numpy().astype(np.int64)
    K = inds.shape[2]
    HW, ld = H * W, case.ld
    kind, tb, tp = mut or (None, -1, -1)
    feat = case.featbuf.numpy().reshape(-1)
    base = HW * ld + FEAT_OFF                                               # the pointer the launch is given
    out = np.full(2 * G + case.out_floats, np.nan, np.float32)
    perm = np.array(row.perm)
    if kind == "perm_inverted":
        inv = np.argsort(perm)
    row0 = 0
    for br, name in enumerate(SPARSE):
        n_out = nout(name, J)
        if br < 3:
            pb = np.repeat(np.arange(B), K)
            ind = inds[:, 0, :].reshape(-1)
        else:
            pb = np.repeat(np.arange(B), J * K)
            ind = inds[:, 1:, :].reshape(-1)
        p = pixel(ind, HW)
        hit = (pb == tb) & (p == tp) if kind else np.zeros(len(p), bool)
        pp = np.where(hit, ind, p) if kind == "no_modulo" else p
        y, x = pp // W, pp % W
        w3 = case.sd[name + ".0.weight"].numpy()
        b3 = case.sd[name + ".0.bias"].numpy()
        w2 = case.sd[name + ".2.weight"].numpy().reshape(n_out, hc)
        b2 = case.sd[name + ".2.bias"].numpy()
        nside = 2 if pairs and br < 2 else 1
        parked = None
        for side in range(nside):
            xs = x
            if side:
                xs = np.where(hit, x, W - 1 - x) if kind == "twin_at_x" else W - 1 - x
            img = (2 * pb + side) if pairs else pb
            if kind == "next_image":
                img = img + hit
            acc = np.zeros((len(p), hc), np.float32)
            for tap in range(9):
                dy, dx = tap // 3 - 1, tap % 3 - 1
                yy, xx = y + dy, xs + dx
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                if kind == "wrap_border":                                   # the flat neighbour, row wrap included
                    q = y * W + xs + dy * W + dx
                    wrap = hit & (q >= 0) & (q < HW)
                    yy, xx, ok = np.where(wrap, q // W, yy), np.where(wrap, q % W, xx), ok | wrap
                stride = np.where(hit, C, ld) if kind == "ld_is_C" else ld
                addr = base + ((img * H + yy) * W + xx) * stride
                addr = np.where(ok, addr, 0)
                a = feat[np.clip(addr[:, None] + np.arange(C)[None, :], 0, feat.size - 1)]
                a = np.where(ok[:, None], a, np.float32(0))
                acc = (acc + a.astype(np.float32) @ w3[:, :, tap // 3, tap % 3].T).astype(np.float32)
            pre = (acc + b3[None, :]).astype(np.float32)
            hid = np.maximum(pre, np.float32(0))
            if kind == "no_relu":
                hid = np.where(hit[:, None], pre, hid)
            rows = np.arange(n_out)
            if side and br == 1:
                rows = 2 * perm[rows >> 1] + (rows & 1)
            v = _one_by_one(hid, w2[rows]) + b2[rows][None, :]
            if side and br == 1 and kind in ("no_perm", "perm_inverted") and hit.any():
                r2 = np.arange(n_out) if kind == "no_perm" else 2 * inv[np.arange(n_out) >> 1] + (np.arange(n_out) & 1)
                v[hit] = (_one_by_one(hid[hit], w2[r2]) + b2[r2][None, :])
            if kind == "drop_hidden" and br == 1 and side == 0:
                j = lowest_spread_row(n_out)
                for i in np.nonzero(hit)[0]:
                    terms = np.abs(hid[i] * w2[j])
                    live = np.nonzero(terms > 0)[0]
                    m = int(live[np.argsort(terms[live])[len(live) // 2]])  # the hidden channel with the median live term
                    v[i, j] = (_one_by_one(hid[i:i + 1], w2[j:j + 1], skip=(0, 0, m)) + b2[j])[0, 0]
            v = v.astype(np.float32)
            if nside == 2:
                if side == 0:
                    parked = v
                    continue
                sign = np.ones((len(p), n_out), np.float32)
                if br == 1:
                    sign[:, 0::2] = -1.0
                    if kind == "sign_on_odd":
                        sign[hit] = -sign[hit]
                a = parked
                if kind == "parked_neighbour":
                    nb = np.arange(len(p))
                    nb = np.where(nb + 1 < len(p), nb + 1, nb - 1)
                    a = np.where(hit[:, None], parked[nb], parked)
                v = ((a + (v * sign).astype(np.float32)).astype(np.float32) / np.float32(2.0)).astype(np.float32)
            at = G + row0 * B * HW + (pb[:, None] * n_out + np.arange(n_out)[None, :]) * HW + pp[:, None]
            inside = (at >= 0) & (at < out.size)
            out[at[inside]] = v[inside]
        row0 += n_out
    return torch.from_numpy(out)


# ---- device runs ------------------------------------------------------------------------------------------------------------------------
def _perm_tensor(perm, dev):
    return torch.tensor(list(perm), dtype=torch.int32, device=dev).view(torch.float32)


def consts(sd, hc, dev):
    """the packed constants of the launchers from a state dict with the four branches under their own names"""
    from centerpose_amd import ops
    w1 = torch.cat([ops.pack_head_points_weight(sd[n + ".0.weight"]) for n in SPARSE]).to(dev)
    b1 = torch.cat([sd[n + ".0.bias"] for n in SPARSE]).to(dev)
    w2 = torch.cat([sd[n + ".2.weight"].reshape(-1, hc) for n in SPARSE]).contiguous().to(dev)
    b2 = torch.cat([sd[n + ".2.bias"] for n in SPARSE]).to(dev)
    return w1, b1, w2, b2


def _launch(case, feat, inds, cst, flat, K):
    from centerpose_amd import ops
    row = case.row
    ws = inds.to(torch.int32).contiguous().view(torch.float32).to(feat.device)
    out = flat[G:G + case.out_floats]
    if case.pairs:
        return ops.head_points_pairs_launch(feat, ws, _perm_tensor(row.perm, feat.device), *cst, out, hc=row.hc, J=row.J, K=K)
    return ops.head_points_launch(feat, ws, *cst, out, hc=row.hc, J=row.J, K=K)


def run_case(cid):
    """one row on the device -> the report of `judge_flat` plus kernel, seconds, rerun_equal, shuffle_equal, relu_share, hps_live, flat"""
    t0 = time.time()
    case = make_case(cid)
    row = case.row
    assert accepted(row) and case.geo["nthr"] <= MAX_THREADS and case.geo["lds"] <= MAX_LDS, cid      # nothing over-wide reaches the device
    dev = torch.device("cuda")
    featbuf = case.featbuf.to(dev)
    feat = featbuf[1:-1, :, :, FEAT_OFF:FEAT_OFF + row.C]
    cst = consts(case.sd, row.hc, dev)
    bits = lambda t: t.cpu().view(torch.int32)

    def once(inds, K):
        flat = torch.full((2 * G + case.out_floats,), float("nan"), device=dev)
        launch = _launch(case, feat, inds, cst, flat, K)
        launch.run()
        torch.cuda.synchronize()
        return flat.cpu(), launch

    flat1, launch = once(case.inds, row.K)
    flat2, _ = once(case.inds, row.K)
    inds2, K2 = shuffled(case.inds, row.H * row.W)
    flat3, _ = once(inds2, K2)
    ref = reference(cid)
    rep = judge_flat(row, case.inds, ref, flat1)
    rep.update(kernel=launch.kernel, rerun_equal=torch.equal(bits(flat1), bits(flat2)), shuffle_equal=torch.equal(bits(flat1), bits(flat3)),
               relu_share=relu_zero_share(case), hps_live=hps_liveness(row, case.inds, ref), flat=flat1, K2=K2,
               featbuf_intact=torch.equal(bits(featbuf), case.featbuf.view(torch.int32)))
    rep["seconds"] = time.time() - t0
    return rep


def dense_merged_by_existing_kernels(cid):
    """MIRROR-3CYC: cp_head_points_f32 at EVERY pixel of the 2N images (K = H W: two dense sets of maps of the existing kernel), merged by
    cp_flip_merge_pairs_f32 -> {name: [N, n, H, W]} (CPU): the direction of the pairs kernel's gather against the dense merge's"""
    from centerpose_amd import ops
    case = make_case(cid)
    row = case.row
    assert case.pairs and row.H * row.W <= 256
    dev = torch.device("cuda")
    feat = case.featbuf.to(dev)[1:-1, :, :, FEAT_OFF:FEAT_OFF + row.C]
    n2, HW, J = case.nimg, row.H * row.W, row.J
    every = torch.arange(HW, dtype=torch.int32).view(1, 1, HW).expand(n2, 1 + J, HW).contiguous()
    dense = torch.full((n2 * HW * (6 + 2 * J),), float("nan"), device=dev)
    ops.head_points_launch(feat, every.view(torch.float32).to(dev), *consts(case.sd, row.hc, dev), dense, hc=row.hc, J=J, K=HW).run()
    srcs, off = [], 0
    for name in SPARSE:
        n = nout(name, J)
        srcs.append(dense[off:off + n2 * n * HW].view(n2, n, row.H, row.W))
        off += n2 * n * HW
    whole = torch.full((row.B * HW * (6 + 2 * J),), float("nan"), device=dev)
    outs, off = [], 0
    for name in SPARSE:
        n = nout(name, J)
        outs.append(whole[off:off + row.B * n * HW].view(row.B, n, row.H, row.W))
        off += row.B * n * HW
    modes = ops.FLIP_MODES
    maps = [(s, o, modes[m]) for s, o, m in zip(srcs, outs, ("flip", "offsets", "copy", "copy"))]
    ops.flip_pairs_launch(maps, whole, _perm_tensor(row.perm, dev)).run()
    torch.cuda.synchronize()
    return {name: o.cpu() for name, o in zip(SPARSE, outs)}


# ---- plans ------------------------------------------------------------------------------------------------------------------------------
# one arch per distinct head geometry (logical C, hc) of layer_oracle.ARCHS: resdcn_50 shares resdcn_18's (64, 64)
PLAN_ARCHS = ("dla_34", "res_50", "hrnet", "mobilenetv3", "shufflenetV2", "resdcn_18")
PLAN_B, PLAN_H, PLAN_W, PLAN_K = 2, 64, 96, 20
PLAN_CASES = [(a, flip) for a in PLAN_ARCHS for flip in (False, True)]


def _pairs_images(n, h, w):
    from centerpose_amd import synth
    img = synth.make_images(n, h, w)
    return torch.stack([img, torch.flip(img, [3])], 1).reshape(2 * n, 3, h, w)


def run_plan_case(arch, flip, seed=317):
    """Engine(dets_only=True) resp. (flip_dets_only=True, 2N = 4) on the spread checkpoint, one step, then the plan's single points
    launch once more on its own from the device inputs the step left (its `feat` view, the `inds` the peak extraction wrote) into a
    NaN-filled output -> the report of `judge_flat` plus kernel, geometry (physical C, hc, featLd), pad_weights_zero, seconds"""
    from centerpose_amd import engine, nets, synth
    t0 = time.time()
    H, W, K = PLAN_H, PLAN_W, PLAN_K
    sd_int = lo.checkpoint(arch, seed, H, W)
    sd_ref = lo.spread_bn(synth.make_state_dict(arch, seed, H=H, W=W))
    if flip:
        eng = engine.Engine(arch, sd_ref, 4, H, W, decode_k=K, flip_dets_only=True, use_graph=False)
        x = _pairs_images(2, H, W).cuda()
    else:
        eng = engine.Engine(arch, sd_ref, PLAN_B, H, W, decode_k=K, dets_only=True, use_graph=False)
        x = synth.make_images(PLAN_B, H, W).cuda()
    eng.process(x)
    torch.cuda.synchronize()
    fn = "cp_head_points_pairs_f32" if flip else "cp_head_points_f32"
    pts = [l for _, _, _, l in eng.launches if l.fn in ("cp_head_points_f32", "cp_head_points_pairs_f32")]
    assert len(pts) == 1 and pts[0].fn == fn, [l.fn for l in pts]
    launch = pts[0]
    feat, ws = launch.tensors[0], launch.tensors[1]
    w1 = launch.tensors[3 if flip else 2]
    ints = launch.ints                                                        # featLd, B or N, H, W, C, J, K, hc
    featLd, n, Hm, Wm, Cp, J, Kp, hc = ints
    C = nets.ARCH_HEAD[arch][0]
    assert (Hm, Wm, Kp, J, hc) == (H // 4, W // 4, K, 17, nets.ARCH_HEAD[arch][1]) and Cp == feat.shape[3] >= C and featLd == feat.stride(2)
    inds = ws.view(torch.int32).cpu()
    row = _r("%s%s" % (arch, "/flip" if flip else ""), "PLAN", B=n, H=Hm, W=Wm, C=C, hc=hc, J=J, K=K,
             perm=[int(v) for v in launch.tensors[2].view(torch.int32).cpu()] if flip else None)
    # the physical channel padding took zero weights: w1 is [4][9][Cp/8][2][hc][4] over k = tap * Cp + c
    wk = w1.cpu().view(4, 9, Cp // 8, 2, hc, 4).permute(0, 1, 2, 3, 5, 4).reshape(4, 9, Cp, hc)
    pad_zero = bool((wk[:, :, C:] == 0).all()) and bool((wk[:, :, :C] != 0).any())
    out = launch.out
    out.fill_(float("nan"))
    launch.run()
    torch.cuda.synchronize()
    flat = torch.cat([torch.full((G,), float("nan")), out.cpu(), torch.full((G,), float("nan"))])
    p = "head" if "head.wh.0.weight" in sd_int else next(k[:-len(".wh.0.weight")] for k in sd_int if k.endswith(".wh.0.weight"))
    sd = {"%s.%s" % (name, s): sd_int["%s.%s.%s" % (p, name, s)] for name in SPARSE for s in ("0.weight", "0.bias", "2.weight", "2.bias")}
    xl = feat.cpu()[..., :C].permute(0, 3, 1, 2).contiguous()
    ref = evaluate(row, flip, xl, sd, f64)
    rep = judge_flat(row, inds, ref, flat)
    rep.update(kernel=launch.kernel, geometry=(Cp, hc, featLd), pad_weights_zero=pad_zero, row=row, inds=inds, ref=ref, seconds=time.time() - t0,
               finite_feat=bool(torch.isfinite(feat).all()))
    return rep


def report_line(tag, rep):
    w = worst_of(rep)
    return "%-28s %-30s worst err / (u A) %7.3f (c = %.2f) at %s %s  %.2f s" % (
        tag, rep["kernel"], w.ratio, rep["c"], [n for n, v in rep["worst"].items() if v is w][0], w.loc, rep["seconds"])
