"""TEST INFRASTRUCTURE ONLY -- per-launch, per-element fp64 oracle of the network plans.

``nets.Graph`` walks every network through its ``emit_*`` hooks and ``engine.PlanBuilder`` turns each hook into one or more
``ops.Launch`` records.  This module

* records which launches every outermost hook call added (``Recording`` / ``RecordingBuilder``),
* restates every hook in plain torch on the CPU (``evaluate``), in float64 (the reference, with the magnitude sum ``A`` of the same
  expression) or in float32 (the independent yardstick the tolerances are calibrated against),
* runs a plan one record at a time on the device and compares every output element with ``|out - ref64| <= c * u * A``
  (``run_plan``; u = 2^-24), each hook judged from its OWN device inputs (teacher forcing: errors do not accumulate),
* walks the same networks on the CPU alone (``CpuWalker``) to measure how far a float32 evaluation -- direct, F(2x2,3x3) and
  F(2x4,3x3) Winograd -- is from the float64 one in the same units: ``LAYER_TOL`` is four times that.

Nothing here reads the device kernels' sources or results to set a bound.  tests/launch_oracle.py judges single forced launches -- the
kernel variants these plans never dispatch to -- with the same pieces.
"""
import collections

import torch
import torch.nn.functional as F

from centerpose_amd import nets, synth
from centerpose_amd.nets import Act
from oracle import dcn as oracle_dcn

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
EPS = 1e-5
ARCHS = ("dla_34", "res_50", "hrnet", "mobilenetv3", "shufflenetV2", "resdcn_18", "resdcn_50")
HOOKS = ("emit_conv", "emit_conv_group", "emit_conv_batch", "emit_maxpool", "emit_dcn", "emit_up_add", "emit_deconv4", "emit_sum_up",
         "emit_sum_up_batch", "emit_head", "emit_dwconv", "emit_se", "emit_scale_add", "emit_shuffle", "emit_half")
SIGMOID_HEADS = ("hm", "hm_hp")
MARGIN = 4.0

# c of `|out - ref64| <= c * u * A` per kernel family = MARGIN x c_ref32.  c_ref32 is the worst err / (u * A) of a plain float32
# torch-CPU evaluation of the same hook against the float64 one, over every record of every arch of ARCHS at B = 2, 64 x 96
# (`calibrate`): the direct evaluation for "direct" and "dcn" (the DCNv2 stage, float32 sampling coordinates included), the textbook
# F(2x2,3x3) / F(2x4,3x3) Winograd (`winograd3x3`, A per tile: `tile_A`) of every 3x3 / s1 / p1 layer for "wino" / "wino24" (the
# fused head kernels are judged as the transform they run).  MARGIN = 4 allows for the MFMA's other summation order and fast
# reciprocals / exponentials.  Measured 2026-10-17 on an x86-64 CPU (torch 2.10 CPU kernels, 8 threads; no GPU involved);
# tests/test_layer_oracle_cpu.py recomputes them and fails when this table is stale.  Worst records: direct = shufflenetV2
# features.14.banch2.5, wino = resdcn_18 layer2.1.conv2, wino24 = dla_34 dla_up.ida_2.proj_2 offset conv, dcn = shufflenetV2
# deconv_layers.0.  A direct-kernel c is additionally capped at K + 3, the worst case of a K-term dot product (`c_for`).
#
# What the bound amounts to next to the plain magnitude sum S = |scale| conv(|x|, |w|) + |shift| + |res| of the one element: direct
# 44 u S = 2.6e-6 S.  Winograd launches take the largest S of the outputs that may share a tile (`tile_A`): 14.4 u resp. 42 u times
# that.  The DCN stage adds 2 (max(H, W) + 2) times the DCN of the 3 x 3 max-pooled |x| for the float32 sampling coordinate
# (`dcn_stage`), 10 x on a 2 x 3 map and 52 x on 16 x 24, so its 5.8 u A is at most about 60 .. 310 u S = 4e-6 .. 2e-5 S.
C_REF32 = {"direct": 10.99, "wino": 3.60, "wino24": 10.49, "dcn": 1.453}
LAYER_TOL = {k: MARGIN * v for k, v in C_REF32.items()}


def c_for(family, K):
    """the constant c for a record of `family` whose every output element is a K-term sum"""
    c = LAYER_TOL[family]
    if family in ("direct", "dcn"):
        c = min(c, K + 3.0)
        assert c <= K + 3.0
    return c


def spread_bn(sd):
    """The one change to the synthetic checkpoint: in every BN weight every fifth channel x 1e-2 and every seventh x 1e+1 -- the
    per-channel scale spread of a trained checkpoint (channels 0, 35, ... get both) -- and the whole vector then divided by the
    RMS of those factors (about 3.5).  The division keeps every ratio between channels and gives the layer back the gain that
    `synth` tuned: without it activations grow about 3.5 x per layer, the offset convs answer with offsets of 1e5 pixels and
    saturated masks, and a DCN samples nothing at all (`dcn_liveness` and `run_plan` assert that this does not happen)."""
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith(".weight") and v.dim() == 1 and k[:-7] + ".running_var" in sd:
            out[k] = v * spread_factors(v.numel()).to(v)
    return out


def spread_factors(n):
    """the per-channel factors of `spread_bn` for n channels (float32), already divided by their RMS: for a launch that has no BN
    (the head branches) the same spread goes on the rows of the weights"""
    f = torch.ones(n)
    f[0::5] *= 1e-2
    f[0::7] *= 1e+1
    return f / f.pow(2).mean().sqrt()


def checkpoint(arch, seed, H, W):
    """the synthetic checkpoint of `arch` with `spread_bn`, under the graph's own key names"""
    return {nets.internal_key(arch, k): v for k, v in spread_bn(synth.make_state_dict(arch, seed, H=H, W=W)).items()}


# ---- recording --------------------------------------------------------------------------------------------------------------------
View = collections.namedtuple("View", "H W C t split")        # an Act without its life-time: holding it never blocks buffer reuse
Record = collections.namedtuple("Record", "hook args out i0 i1")


def _views(o):
    if isinstance(o, Act):
        return View(o.H, o.W, o.C, o.t, o.split)
    if isinstance(o, (list, tuple)):
        return type(o)(_views(v) for v in o)
    return o


class Recording:
    """Mix-in in front of a `nets.Graph`: every OUTERMOST emit_* call appends Record(hook, args, returned Act(s), i0, i1) with
    [i0, i1) the range of `self.launches` the call added (hooks called from inside a hook -- emit_se -> emit_conv, a grouped hook
    falling back to single ones -- belong to the outer record)."""

    def _record(self, hook, args, call):
        if getattr(self, "_depth", 0):
            return call()
        if not hasattr(self, "records"):
            self.records = []
        self._depth = 1
        i0 = len(getattr(self, "launches", ()))
        try:
            out = call()
        finally:
            self._depth = 0
        self.records.append(Record(hook, _views(args), _views(out), i0, len(getattr(self, "launches", ()))))
        return out


def _make_hook(name):
    def hook(self, *args):
        return self._record(name, args, lambda: getattr(super(Recording, self), name)(*args))
    hook.__name__ = name
    return hook


for _h in HOOKS:
    setattr(Recording, _h, _make_hook(_h))


class SpecRecorder(Recording, nets.Graph):
    """shape-only walk (no device): the bookkeeping of `Recording` on its own"""
    launches = ()


def recording_builder():
    """RecordingBuilder: engine.PlanBuilder behind `Recording` (imported late: the engine needs the HIP library)."""
    from centerpose_amd import engine

    class RecordingBuilder(Recording, engine.PlanBuilder):
        pass
    return RecordingBuilder


def check_partition(records, nlaunches):
    """every launch of the plan belongs to exactly one record"""
    seen = [0] * nlaunches
    for r in records:
        for i in range(r.i0, r.i1):
            seen[i] += 1
    assert all(s == 1 for s in seen), "launches not covered exactly once: %s" % [i for i, s in enumerate(seen) if s != 1][:8]


# ---- plain-torch hooks --------------------------------------------------------------------------------------------------------------
class Out:
    """one output of a hook: value, magnitude sum A (float64 evaluations only), K terms per element, exact (must be bit-equal to
    the float32 evaluation), hsig (h-sigmoid epilogue: padding channels hold 0.5)"""

    def __init__(self, val, A=None, K=1, exact=False, hsig=False):
        self.val, self.A, self.K, self.exact, self.hsig = val, A, K, exact, hsig


def _fold(sd, bn, bias, co, dt):
    """(scale, shift, A of the shift's own terms) of BN(conv + bias), evaluated in `dt` from the float32 parameters"""
    b = sd[bias].to(dt) if bias else None
    if bn:
        g, beta, mean, var = (sd["%s.%s" % (bn, s)].to(dt) for s in ("weight", "bias", "running_mean", "running_var"))
        scale = g / torch.sqrt(var + EPS)
        shift = beta - mean * scale
        ash = beta.abs() + (mean * scale).abs()
        if b is not None:
            shift = shift + b * scale
            ash = ash + (b * scale).abs()
    else:
        scale = torch.ones(co, dtype=dt)
        shift = b.clone() if b is not None else torch.zeros(co, dtype=dt)
        ash = shift.abs()
    v = lambda t: t.view(1, -1, 1, 1)
    return v(scale), v(shift), v(ash)


def _activate(v, A, act):
    """activation and what it does to the magnitude sum: a few ulps of the result plus |d act / dv| x the error of v"""
    if act in (True, "relu"):
        return F.relu(v), A
    if act == "hswish":
        o = v * F.relu6(v + 3) / 6
        return o, None if A is None else 1.5 * A + o.abs()
    if act == "hsigmoid":
        o = F.relu6(v + 3) / 6
        return o, None if A is None else (A + 3) / 6 + o.abs()
    if act == "sigmoid":
        o = torch.sigmoid(v)
        return o, None if A is None else o * (1 - o) * A + o
    assert act in (False, None), act
    return v, A


WINO = {   # textbook transforms (Lavin & Gray 2016): F(2,3) and F(4,3) with the points 0, +-1, +-2
    2: (torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64),
        torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64),
        torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)),
    4: (torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                      [0, 4, 0, -5, 0, 1]], dtype=torch.float64),
        torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                      [0, 0, 1]], dtype=torch.float64),
        torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)),
}


def winograd3x3(x, w, mh, mw):
    """3x3 / stride 1 / pad 1 convolution as F(mh x mw, 3x3) Winograd in x.dtype; weights transformed in float64 and rounded once."""
    (BTh, Gh, ATh), (BTw, Gw, ATw) = WINO[mh], WINO[mw]
    dt = x.dtype
    B, C, H, W = x.shape
    th, tw = -(-H // mh), -(-W // mw)
    Uw = torch.einsum("ai,ocij,bj->ocab", Gh, w.double(), Gw).to(dt)
    xp = F.pad(x, (1, tw * mw - W + 1, 1, th * mh - H + 1))
    d = xp.unfold(2, mh + 2, mh).unfold(3, mw + 2, mw)                     # [B, C, th, tw, mh+2, mw+2]
    V = torch.einsum("ai,bcyxij,ej->bcyxae", BTh.to(dt), d, BTw.to(dt))
    M = torch.einsum("ocae,bcyxae->boyxae", Uw, V)
    Y = torch.einsum("ia,boyxae,je->boyxij", ATh.to(dt), M, ATw.to(dt))    # [B, O, th, tw, mh, mw]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], th * mh, tw * mw)[:, :, :H, :W].contiguous()


def _conv(x, w, stride, pad, groups, wino, dt):
    if wino and w.shape[2] == 3 and stride == 1 and pad == 1 and groups == 1:
        return winograd3x3(x, w, 2, 4 if wino == "wino24" else 2)
    return F.conv2d(x, w, None, stride, pad, 1, groups)


def _affine(x, Ax, w, scale, shift, ash, res=None, act=None, stride=1, pad=0, groups=1, wino=None, extra=4):
    """act(conv(x, w) * scale + shift (+ res)) -> Out; A = |scale| conv(Ax, |w|) + |shift terms| + |res| (Ax >= |x|: the input's own
    magnitude sum when it is an intermediate of the same hook)"""
    dt = x.dtype
    w = w.to(dt)
    v = _conv(x, w, stride, pad, groups, wino, dt) * scale + shift
    A = None
    if dt == torch.float64:
        A = scale.abs() * F.conv2d(Ax, w.abs(), None, stride, pad, 1, groups) + ash
    if res is not None:
        v = v + res
        A = None if A is None else A + res.abs()
    v, A = _activate(v, A, act)
    return Out(v, A, w.shape[1] * w.shape[2] * w.shape[3] + extra)


def _conv_bn(sd, x, conv, bn, bias, co, k, stride, pad, relu, res, dt, wino=None):
    scale, shift, ash = _fold(sd, bn, conv + ".bias" if bias else None, co, dt)
    return _affine(x, x.abs(), sd[conv + ".weight"], scale, shift, ash, res, relu, stride, pad, wino=wino)


def _up(x, sh):
    return F.interpolate(x, scale_factor=2 ** sh, mode="nearest") if sh else x


def _sum_up(xs, shifts, relu):
    ts = [_up(x, s) for x, s in zip(xs, shifts)]
    v = ts[0]
    for t in ts[1:]:
        v = v + t
    A = sum(t.abs() for t in ts) if v.dtype == torch.float64 else None
    return Out(F.relu(v) if relu else v, A, len(ts))


def dcn_stage(sd, x, om, conv, bn, co, dt, extent=None):
    """DCNv2 + bias + BN + ReLU from x and the given offset / mask logits `om` [B, 27, H, W] (teacher-forced: sampling is
    discontinuous in the offsets).  The sampling coordinate y + ky + offset is one float32 rounding away from its float64 value,
    <= u |coordinate| with |coordinate| < max(H, W) + 2 for every sample that contributes, and a bilinear sample moves by at most
    (|dy| + |dx|) x 2 x the largest of its four corners: A carries P x the same DCN over the 3 x 3 max-pooled |x| (>= every corner).
    extent: max(H, W) of the map the device launch samples when `x` is only a crop of it (tests/limit_oracle.py): the device forms its
    coordinates in the whole map."""
    B, C, H, W = x.shape
    om = om.to(dt)
    off, mask = om[:, :18].contiguous(), torch.sigmoid(om[:, 18:27]).contiguous()
    w = sd[conv + ".weight"].to(dt)
    scale, shift, ash = _fold(sd, bn, conv + ".bias", co, dt)
    v = oracle_dcn.dcn_v2_forward_torch(x, w, None, off, mask) * scale + shift
    A = None
    if dt == torch.float64:
        P = 2.0 * ((extent or max(H, W)) + 2)
        a = oracle_dcn.dcn_v2_forward_torch(x.abs() + P * F.max_pool2d(x.abs(), 3, 1, 1), w.abs(), None, off, mask)
        A = scale.abs() * a + ash
    return Out(F.relu(v), A, 9 * C + 4)


def head_branch(sd, xv, c3, c1, hc, n, act, dt, wino=None):
    """one KeypointHead branch: conv3x3 `c3` + bias + ReLU -> conv1x1 `c1` + bias (+ `act`) of xv (already in `dt`) -> Out; K counts both
    sums, A carries the mid activations' own magnitude sums through the 1x1"""
    mid = _affine(xv, xv.abs(), sd[c3 + ".weight"], *_fold(sd, None, c3 + ".bias", hc, dt), act=True, pad=1, wino=wino)
    o = _affine(mid.val, mid.A if mid.A is not None else mid.val.abs(), sd[c1 + ".weight"], *_fold(sd, None, c1 + ".bias", n, dt), act=act)
    o.K += mid.K
    return o


def evaluate(hook, sd, args, get, dt, wino=None, om=None):
    """The hook `hook(*args)` in plain torch, dtype `dt`.  `get(view, nchw=False)` -> the input's LOGICAL channels as a float32 NCHW
    CPU tensor.  -> [Out] in the order of the hook's outputs.  wino: None (direct) / "wino" / "wino24": how 3x3 / s1 / p1 convs are
    evaluated (float32 calibration only).  om (emit_dcn): the offset / mask logits the DCN stage samples with."""
    g = lambda a, nchw=False: get(a, nchw).to(dt)
    if hook == "emit_conv":
        xs, conv, bn, bias, co, k, stride, pad, relu, res, stem = args
        x = torch.cat([g(a, stem) for a in xs], 1)
        return [_conv_bn(sd, x, conv, bn, bias, co, k, stride, pad, relu, g(res) if res is not None else None, dt, wino)]
    if hook == "emit_conv_group":
        return [_conv_bn(sd, g(x), conv, bn, False, co, 3, 1, 1, relu, g(res) if res is not None else None, dt, wino)
                for x, conv, bn, co, relu, res in args[0]]
    if hook == "emit_conv_batch":
        return [_conv_bn(sd, g(x), conv, bn, False, co, k, stride, pad, relu, None, dt, wino)
                for x, conv, bn, co, k, stride, pad, relu in args[0]]
    if hook == "emit_maxpool":
        x, k, s, p = args
        return [Out(F.max_pool2d(g(x), k, s, p), exact=True)]
    if hook == "emit_dcn":
        x, conv, bn, co = args
        xv = g(x)
        scale, shift, ash = _fold(sd, None, conv + ".conv_offset_mask.bias", 27, dt)
        o1 = _affine(xv, xv.abs(), sd[conv + ".conv_offset_mask.weight"], scale, shift, ash, pad=1, wino=wino)
        return [o1, dcn_stage(sd, xv, om if om is not None else o1.val.float(), conv, bn, co, dt)]
    if hook == "emit_up_add":
        x, wname, f, add = args
        xv, w, av = g(x), sd[wname + ".weight"].to(dt), g(add)
        ct = lambda t, ww: F.conv_transpose2d(t, ww, None, stride=f, padding=f // 2, groups=t.shape[1])
        return [Out(ct(xv, w) + av, ct(xv.abs(), w.abs()) + av.abs() if dt == torch.float64 else None, 5)]
    if hook == "emit_deconv4":
        x, wname, bn, co = args
        xv, w = g(x), sd[wname + ".weight"].to(dt)
        scale, shift, ash = _fold(sd, bn, None, co, dt)
        v = F.conv_transpose2d(xv, w, None, 2, 1) * scale + shift
        A = scale.abs() * F.conv_transpose2d(xv.abs(), w.abs(), None, 2, 1) + ash if dt == torch.float64 else None
        return [Out(F.relu(v), A, 4 * w.shape[0] + 4)]
    if hook == "emit_sum_up":
        xs, shifts, relu = args
        return [_sum_up([g(a) for a in xs], shifts, relu)]
    if hook == "emit_sum_up_batch":
        return [_sum_up([g(a) for a in xs], shifts, args[1]) for xs, shifts in args[0]]
    if hook == "emit_dwconv":
        x, conv, bn, k, stride, act = args
        xv = g(x)
        scale, shift, ash = _fold(sd, bn, None, xv.shape[1], dt)
        return [_affine(xv, xv.abs(), sd[conv + ".weight"], scale, shift, ash, None, act, stride, k // 2, groups=xv.shape[1])]
    if hook == "emit_se":
        x, p, red = args
        xv = g(x)
        hw = xv.shape[2] * xv.shape[3]
        pooled, apool = xv.sum((2, 3), keepdim=True) / hw, xv.abs().sum((2, 3), keepdim=True) / hw
        mid = _affine(pooled, apool, sd[p + ".1.weight"], *_fold(sd, p + ".2", None, red, dt), act=True)
        out = _affine(mid.val, mid.A if mid.A is not None else mid.val.abs(), sd[p + ".4.weight"], *_fold(sd, p + ".5", None, xv.shape[1], dt),
                      act="hsigmoid")
        out.K, out.hsig = hw + red + 8, True
        return [out]
    if hook == "emit_scale_add":
        x, se, add = args
        xv, sv = get(x, False), get(se, False)
        if add is None:
            return [Out((xv * sv).to(dt), exact=True)]
        # two roundings.  Not because of a build flag: seven objects of csrc/Makefile are built with -ffp-contract=off, elementwise.o is
        # not (it would change the bits of DLA-34's up-sampling).  scale_add_kernel forms the float4 product as one statement and adds
        # the addend in a later, conditional one, and the compiler keeps them apart (a packed multiply, then a packed add); should a
        # compiler ever fuse them, the two roundings are to be made explicit in that kernel, not loosened here.
        # tests/test_helper_parity_hip.py holds the kernel to the same two roundings over multi-block rows and strided views.
        return [Out((xv * sv + get(add, False)).to(dt), exact=True)]
    if hook == "emit_shuffle":
        x1, x2 = args
        c = torch.cat([g(x1), g(x2)], 1)
        b, ch, h, w = c.shape
        return [Out(c.view(b, 2, ch // 2, h, w).transpose(1, 2).reshape(b, ch, h, w), exact=True)]
    if hook == "emit_half":
        x, which = args
        h = x.split[0]
        return [Out(g(x)[:, which * h:(which + 1) * h], exact=True)]
    if hook == "emit_head":
        feat, p, hc = args
        xv = g(feat)
        return [head_branch(sd, xv, "%s.%s.0" % (p, h), "%s.%s.2" % (p, h), hc, n, "sigmoid" if h in SIGMOID_HEADS else None, dt, wino)
                for h, n in nets.HEADS]
    raise ValueError(hook)


# ---- comparator -------------------------------------------------------------------------------------------------------------------
Worst = collections.namedtuple("Worst", "ratio loc err A")


def worst_ratio(out, ref64, A):
    """worst err_i / (u A_i) over the tensor and where: Worst(ratio, (b, c, y, x), err, A).  An element with A = 0 has nothing to
    round: any error there is infinite."""
    err = (out.double() - ref64).abs()
    err = (err - FLT_MIN).clamp_(min=0.0)            # a float32 result below the smallest normal number may flush to zero
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * A))
    ratio = torch.where(torch.isfinite(out.double()) & torch.isfinite(ref64), ratio, torch.full_like(ratio, float("inf")))
    i = int(torch.argmax(ratio))
    loc = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return Worst(float(ratio.reshape(-1)[i]), loc, float(err.reshape(-1)[i]), float(A.reshape(-1)[i]))


def first_unequal(out, want):
    """location of the first element of `out` that differs from `want`, or None"""
    bad = out != want
    if not bool(bad.any()):
        return None
    return tuple(int(v) for v in torch.unravel_index(torch.argmax(bad.reshape(-1).to(torch.uint8)), bad.shape))


def logical(t, view):
    """physical NHWC tensor of `view` -> its logical channels, NCHW"""
    return t[..., cmap(view)].permute(0, 3, 1, 2).contiguous()


def cmap(a):
    if a.split:
        h, hp = a.split
        return list(range(h)) + list(range(hp, hp + h))
    return list(range(a.C))


def padding_violation(t, view, hsig=False):
    """location (b, y, x, physical channel) of the first padding channel of the physical NHWC tensor that is not exactly zero (0.5 after
    an h-sigmoid epilogue: h-sigmoid(0)), or None"""
    pad = sorted(set(range(t.shape[3])) - set(cmap(view)))
    if not pad:
        return None
    bad = t[..., pad] != (0.5 if hsig else 0.0)
    if hsig:
        bad &= t[..., pad] != 0.0
    if not bool(bad.any()):
        return None
    b, y, x, c = (int(v) for v in torch.unravel_index(torch.argmax(bad.reshape(-1).to(torch.uint8)), bad.shape))
    return (b, y, x, pad[c])


def tile_A(A, family):
    """A Winograd kernel forms every output of a 2 x 2 (F(2x2,3x3)) or 2 x 4 (F(2x4,3x3)) tile from sums over the tile's whole input
    patch, so its rounding error follows the magnitude of the tile, not of the one 3 x 3 window: A_i of such a launch is the largest A
    over the outputs that can share a tile with i (tile alignment left open: 3 x 3 resp. 3 x 7 outputs around i)."""
    if family not in ("wino", "wino24") or A.dim() != 4:
        return A
    mw = 4 if family == "wino24" else 2
    return F.max_pool2d(A, (3, 2 * mw - 1), 1, (1, mw - 1))


def judge(out32, o32, o64, family):
    """-> (Worst or None, failure text or None) for one output: device (or stand-in) value `out32` against the float32 evaluation
    `o32` (exact hooks) or the float64 one `o64` with its A."""
    if o64.exact:
        loc = first_unequal(out32, o32.val)
        return None, None if loc is None else "not bit-equal to the float32 reference at %s: %r != %r" % (loc, float(out32[loc]), float(o32.val[loc]))
    w = worst_ratio(out32, o64.val, tile_A(o64.A, family))
    c = c_for(family, o64.K)
    return w, None if w.ratio <= c else "err %.3e = %.1f u A (A = %.3e) > c = %.1f at (b, c, y, x) = %s" % (w.err, w.ratio, w.A, c, w.loc)


# ---- liveness: the data must exercise what the records are there to check ---------------------------------------------------------------
# Floors on the test's own data, not on the kernels.  A DCN whose samples all fall outside the map, or whose masks are all 0 or 1, puts
# out ReLU(shift) whatever its sampling code does; a sigmoid head that is 0 or 1 everywhere checks no sigmoid.  With zero offsets the
# 2 x 3 map -- the smallest here -- has 14/27 of its 3 x 3 taps inside (2/3 of the rows times 7/9 of the columns), and `synth` sends
# every third DCN's tap far outside on purpose, so a tenth of the samples is asked for; half of the masks must lie in (0.01, 0.99), and a
# tenth of every sigmoid map in (1e-6, 1 - 1e-6), the range in which float32 still resolves the slope of the sigmoid.
LIVE_FLOOR = {"dcn_samples": 0.1, "dcn_masks": 0.5, "sigmoid": 0.1}


def dcn_liveness(om):
    """(fraction of the 9 H W samples that fall inside the map, fraction of masks in (0.01, 0.99)) for offset / mask logits [B, 27, H, W]"""
    B, _, H, W = om.shape
    om = om.double()
    off = om[:, :18].view(B, 9, 2, H, W)
    k = torch.arange(9)
    h = torch.arange(H).view(1, 1, H, 1) - 1.0 + (k // 3).view(1, 9, 1, 1) + off[:, :, 0]
    w = torch.arange(W).view(1, 1, 1, W) - 1.0 + (k % 3).view(1, 9, 1, 1) + off[:, :, 1]
    m = torch.sigmoid(om[:, 18:27])
    return (float(((h > -1) & (w > -1) & (h < H) & (w < W)).double().mean()), float(((m > 0.01) & (m < 0.99)).double().mean()))


def sigmoid_liveness(v):
    """fraction of a sigmoid map in (1e-6, 1 - 1e-6)"""
    return float(((v > 1e-6) & (v < 1 - 1e-6)).double().mean())


def liveness(hook, vals, om=None):
    """{key of LIVE_FLOOR: fraction} of one record: `om` the logits an emit_dcn samples with, `vals` the outputs of an emit_head"""
    if hook == "emit_dcn":
        return dict(zip(("dcn_samples", "dcn_masks"), dcn_liveness(om)))
    if hook == "emit_head":
        return {"sigmoid": min(sigmoid_liveness(v) for (h, _), v in zip(nets.HEADS, vals) if h in SIGMOID_HEADS)}
    return {}


def note_liveness(live, failures, label, hook, vals, om=None):
    """fold one record's fractions into `live` {key: (lowest fraction, its record)}; a fraction under its floor is a failure"""
    for key, frac in liveness(hook, vals, om).items():
        if frac < live.get(key, (2.0, ""))[0]:
            live[key] = (frac, label)
        if frac < LIVE_FLOOR[key]:
            failures.append("%s: degenerate test data: %s = %.3f < %.2f" % (label, key, frac, LIVE_FLOOR[key]))


# ---- CPU walk: calibration --------------------------------------------------------------------------------------------------------
class CpuWalker(nets.Graph):
    """Walks a network on the CPU in float32 (every Act.t = logical NCHW tensor) and measures, hook by hook, the float32 evaluations
    against the float64 one from the same inputs: `self.c_ref32[family]` = worst err / (u A), `self.where[family]` its record."""

    def __init__(self, sd):
        super().__init__()
        self.sd = sd
        self.c_ref32 = dict.fromkeys(LAYER_TOL, 0.0)
        self.where = {}
        self.nrec = 0
        self.maxabs = 0.0
        self.outputs = None
        self.live, self.dead = {}, []

    def _note(self, family, name, o32, o64):
        for a, b in zip(o32, o64):
            if b.exact:
                assert first_unequal(a.val.float(), b.val.float()) is None, name
                continue
            w = worst_ratio(a.val, b.val, tile_A(b.A, family))
            if w.ratio > self.c_ref32[family]:
                self.c_ref32[family], self.where[family] = w.ratio, (name, w.loc)

    def _walk(self, hook, args):
        sd, get = self.sd, lambda a, nchw=False: a.t
        o32 = evaluate(hook, sd, args, get, torch.float32)
        om = o32[0].val if hook == "emit_dcn" else None
        o64 = evaluate(hook, sd, args, get, torch.float64, om=om)
        name = "%s(%s)" % (hook, next((a for a in _flat(args) if isinstance(a, str)), ""))
        self.nrec += 1
        if hook == "emit_dcn":
            self._note("direct", name, o32[:1], o64[:1])
            self._note("dcn", name, o32[1:], o64[1:])
        else:
            self._note("direct", name, o32, o64)
        for fam in ("wino", "wino24"):
            if _has_wino_conv(hook, args):
                ow = evaluate(hook, sd, args, get, torch.float32, wino=fam, om=om)
                self._note(fam, name, ow[:1] if hook == "emit_dcn" else ow, o64[:1] if hook == "emit_dcn" else o64)
        vals = [o.val.float() for o in o32]
        note_liveness(self.live, self.dead, name, hook, vals, om)
        self.maxabs = max([self.maxabs] + [float(v.abs().max()) for v in vals])
        return vals

    @staticmethod
    def _act(v, split=None):
        return Act(v.shape[2], v.shape[3], v.shape[1], v, split)

    def emit_head(self, *args):
        self.outputs = self._walk("emit_head", args)

    def emit_dcn(self, *args):
        return self._act(self._walk("emit_dcn", args)[1])

    def emit_shuffle(self, x1, x2):
        return self._act(self._walk("emit_shuffle", (x1, x2))[0], (x1.C, (x1.C + 15) // 16 * 16))

    def emit_dwconv(self, x, *args):
        return self._act(self._walk("emit_dwconv", (x,) + args)[0], x.split)


def _single(name):
    def hook(self, *args):
        return self._act(self._walk(name, args)[0])
    return hook


def _multi(name):
    def hook(self, *args):
        return [self._act(v) for v in self._walk(name, args)]
    return hook


for _h in ("emit_conv", "emit_maxpool", "emit_up_add", "emit_deconv4", "emit_sum_up", "emit_se", "emit_scale_add", "emit_half"):
    setattr(CpuWalker, _h, _single(_h))
for _h in ("emit_conv_group", "emit_conv_batch", "emit_sum_up_batch"):
    setattr(CpuWalker, _h, _multi(_h))


def _flat(o):
    if isinstance(o, (list, tuple)) and not isinstance(o, View):
        for v in o:
            yield from _flat(v)
    else:
        yield o


def _has_wino_conv(hook, args):
    """does the hook hold a 3x3 / stride-1 / pad-1 convolution a Winograd kernel may take (>= 17 logical = 32 physical input channels)"""
    if hook == "emit_conv":
        xs, _, _, _, _, k, stride, pad, _, _, stem = args
        return k == 3 and stride == 1 and pad == 1 and len(xs) == 1 and not stem and xs[0].C > 16
    if hook == "emit_conv_group":
        return all(m[0].C > 16 for m in args[0])
    if hook in ("emit_dcn", "emit_head"):
        return args[0].C > 16
    return False


def calibrate(archs=ARCHS, B=2, H=64, W=96, seed=317):
    """c_ref32 per family over every record of every arch (CPU only) -> (dict family -> c_ref32, dict family -> (arch, record, loc))"""
    c, where = dict.fromkeys(LAYER_TOL, 0.0), {}
    with torch.no_grad():
        for arch in archs:
            wk = CpuWalker(checkpoint(arch, seed, H, W))
            wk.network(arch, Act(H, W, 3, synth.make_images(B, H, W)))
            assert wk.maxabs < 1e3 and all(bool(torch.isfinite(o).all()) for o in wk.outputs), (arch, wk.maxabs)   # activations stay O(1)
            assert not wk.dead, wk.dead
            for fam, v in wk.c_ref32.items():
                if v > c[fam]:
                    c[fam], where[fam] = v, (arch,) + wk.where[fam]
    return c, where


# ---- device run -------------------------------------------------------------------------------------------------------------------
def _family(kinds):
    return "wino24" if "wino24" in kinds else "wino" if "wino" in kinds else "direct"


def run_plan(arch, B, H, W, seed=317, device="cuda"):
    """Build the plan of `arch` behind a RecordingBuilder and run it record by record.  -> dict(launches, checked, kernels (set of
    device kernel names), worst {family: (ratio, text)}, failures [text], launch_list [`_launch_facts`])."""
    sd = checkpoint(arch, seed, H, W)
    dev = torch.device(device)
    images = synth.make_images(B, H, W).to(dev)
    with torch.cuda.device(dev):
        pb = recording_builder()(sd, B, dev)
        pb.network(arch, Act(H, W, 3, images))
    check_partition(pb.records, len(pb.launches))
    rep = dict(launches=len(pb.launches), checked=0, kernels=set(), worst={}, failures=[], records=len(pb.records), live={})
    with torch.no_grad():
        for rec in pb.records:
            ins = [a for a in _flat(rec.args) if isinstance(a, View)]
            snap = {id(a): a.t.clone() for a in ins}          # `out` may alias an input (emit_up_add), pool slots are reused
            ll = pb.launches[rec.i0:rec.i1]
            for _, _, _, launch in ll:
                launch.run()
            torch.cuda.synchronize(dev)
            rep["checked"] += len(ll)
            names = [launch.kernel for _, _, _, launch in ll]
            rep["kernels"].update(names)
            if rec.hook == "emit_maxpool" and not ll:
                continue                                      # a DLA tree's cached pooling: the Act of an earlier record
            get = lambda a, nchw=False: snap[id(a)].cpu() if nchw else logical(snap[id(a)].cpu(), a)
            outs, om = _device_outputs(pb, rec, ll)
            o32 = evaluate(rec.hook, sd, rec.args, get, torch.float32, om=om)
            o64 = evaluate(rec.hook, sd, rec.args, get, torch.float64, om=om)
            label = "%s %s(%s) launches %d..%d" % (arch, rec.hook, next((a for a in _flat(rec.args) if isinstance(a, str)), ""), rec.i0, rec.i1 - 1)
            note_liveness(rep["live"], rep["failures"], label, rec.hook, [t.cpu() for _, t in outs], om)
            for j, ((view, t), a, b) in enumerate(zip(outs, o32, o64)):
                fam, kn = _family([k for k, _, _, _ in ll]), names
                if rec.hook == "emit_dcn":                    # two stages, each with its own launches
                    split = next(i for i, (k, _, _, _) in enumerate(ll) if k == "dcn")
                    part = ll[:split] if j == 0 else ll[split:]
                    fam, kn = (_family([k for k, _, _, _ in part]) if j == 0 else "dcn"), [l.kernel for _, _, _, l in part]
                t = t.cpu()
                if view is not None:
                    loc = padding_violation(t, view, b.hsig)
                    if loc is not None:
                        rep["failures"].append("%s [%s]: padding channel not zero at (b, y, x, c) = %s: %r" % (label, ",".join(kn), loc, float(t[loc])))
                    t = logical(t, view)
                w, fail = judge(t, a, b, fam)
                if w is not None and w.ratio > rep["worst"].get(fam, (-1.0, ""))[0]:
                    rep["worst"][fam] = (w.ratio, "%s [%s] at %s" % (label, ",".join(sorted(set(kn))), w.loc))
                if fail:
                    rep["failures"].append("%s output %d [%s]: %s" % (label, j, ",".join(kn), fail))
    rep["launch_list"] = [_launch_facts(name, launch) for _, name, _, launch in pb.launches]
    return rep


def _launch_facts(name, launch):
    """what a dispatch rule looks at, without holding the launch's buffers: dict(name, fn, kernel) and, for cp_conv2d_f32, the descriptor
    fields and whether every source is 16-byte aligned"""
    f = dict(name=name, fn=launch.fn, kernel=launch.kernel)
    if launch.fn == "cp_conv2d_f32":
        d = launch.desc
        f.update({k: getattr(d, k) for k in ("tile", "inNCHW", "ldw", "nsrc", "kh", "kw", "Cout", "ksplit", "nsub")})
        f.update(srcC0=d.srcC[0], aligned=all(t.data_ptr() % 16 == 0 for t in launch.tensors[:d.nsrc]))
    return f


def _device_outputs(pb, rec, ll):
    """[(view or None for an NCHW head map, device tensor)] in the order of `evaluate`'s outputs, and the DCN's own offset / mask
    logits (logical, CPU) when the record is an emit_dcn"""
    if rec.hook == "emit_head":
        return [(None, t) for t in pb.outputs], None
    if rec.hook == "emit_dcn":
        omt = next(l for k, _, _, l in ll if k == "dcn").reads[1]          # the buffer the DCN launch itself samples with
        omv = View(omt.shape[1], omt.shape[2], 27, omt, None)
        return [(omv, omt), (rec.out, rec.out.t)], logical(omt.cpu(), omv)
    outs = rec.out if isinstance(rec.out, (list, tuple)) and not isinstance(rec.out, View) else [rec.out]
    return [(v, v.t) for v in outs], None


def format_report(tag, rep):
    lines = ["%s: %d launches in %d records, %d checked" % (tag, rep["launches"], rep["records"], rep["checked"]),
             "  kernels: " + ", ".join(sorted(rep["kernels"]))]
    for fam, (ratio, text) in sorted(rep["worst"].items()):
        lines.append("  worst err / (u A) %-7s %8.3f (LAYER_TOL %.1f)  %s" % (fam, ratio, LAYER_TOL[fam], text))
    for key, (frac, text) in sorted(rep["live"].items()):
        lines.append("  lowest live fraction %-12s %.3f (floor %.2f)  %s" % (key, frac, LIVE_FLOOR[key], text))
    return "\n".join(lines)
