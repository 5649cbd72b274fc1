"""The k-loops of `igemm_conv_kernel` / `igemm_conv_group_kernel` and `dcn_igemm_kernel` run unrolled by two on compile-time LDS
buffers (an odd count of k-steps takes its first step out of buffer 1), the gathers and the weight slices go through a scalar base plus
a 32-bit lane offset, and the generic kernel forms the tap part of a gather offset on the scalar unit.  What can go wrong there is the
buffer a step reads or stages into, the parity of a split-K range, the segment start of a tap or of a concatenated source, and the
zero-select of a border tap -- all of which change the answer by whole terms.  So the generic and the DCNv2 cases below use data on which
float32 is EXACT (small integers; bilinear corner weights 0, 1/4, 1/2, 1; masks 0, 1/2, 1) and compare `==`:

* generic kernel against a float64 torch-CPU convolution: 1, 2, 3, 5 k-steps; a stride-2 3x3 on a 9 x 11 map (border taps invalid on
  all four sides); Root-style 1x1 with 2 and 3 sources of different channel counts; M no multiple of 64; split-K with S = 2, 3 over
  9 k-steps (3x3 x 16 channels, and 1x3 x 48 channels where S = 2 starts inside a tap) + `cp_splitk_reduce_f32`; one
  `cp_conv2d_group_f32` launch with two members of different K;
* DCNv2 against oracle/dcn_ref.c (double accumulation): C = 16, 32, 48 (1, 2, 3 k-steps per tap), ksplit 1 and 3, tiles 64 x 64 and
  64 x 128 (ldw = 128), offsets on the half-integer grid that leave the map on every side.

The F(2x4) convolution (single and grouped launch) and the fused head kernels are run at the smallest shapes that reach their odd
stage tail, ragged tiles, both epilogues and all five head instantiations, against the float64 oracle at its existing bound
(tests/launch_oracle.py; no tolerance of this file's own), the heads under both `CP_HEAD_STAGGER` settings bit for bit.

Every case runs twice and must give equal bits.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launch_oracle as L
import layer_oracle as lo

pytestmark = pytest.mark.gpu

IG64 = "igemm_conv_kernel<64, 64, 2, 2, 32, false>"
IG128 = "igemm_conv_kernel<128, 64, 2, 2, 32, false>"
TILES = {64064: IG64, 128064: IG128}


def _ints(g, shape, lo_, hi):
    return torch.randint(lo_, hi + 1, shape, generator=g).float()


def _dev_nhwc(t, extra=0):
    """logical NCHW CPU tensor -> device NHWC view with `extra` more floats per pixel behind the channels"""
    B, C, H, W = t.shape
    buf = torch.zeros(B, H, W, C + extra, device="cuda")
    buf[..., :C] = t.permute(0, 2, 3, 1).cuda()
    return buf[..., :C]


def _twice(launches, read):
    for l in launches:
        l.run()
    torch.cuda.synchronize()
    first = read()
    for l in launches:
        l.run()
    torch.cuda.synchronize()
    second = read()
    bits = lambda t: t.contiguous().view(torch.int32)                      # the NaN guards compare as bits too
    assert torch.equal(bits(first), bits(second)), "a second run gives other bits at %s" % (lo.first_unequal(bits(first), bits(second)),)
    return first


# ---- generic implicit GEMM: exact answers -------------------------------------------------------------------------------------------
def _conv_exact(seed, srcC, cout, kh, kw, stride, pad_yx, B, H, W, tile, S=1):
    """one forced launch of the generic kernel on integer data -> (kernel name, device result NCHW float64, float64 reference)"""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(seed)
    xs = [_ints(g, (B, c, H, W), -3, 3) for c in srcC]
    w = _ints(g, (cout, sum(srcC), kh, kw), -2, 2)
    bias = _ints(g, (cout,), -5, 5)
    ref = F.conv2d(torch.cat(xs, 1).double(), w.double(), bias.double(), stride=stride, padding=pad_yx)
    Ho, Wo = ref.shape[2:]
    wp = ops.pack_conv_weight(w.cuda())
    ldw = wp.shape[0]
    sc, sh = ops.fold_bn(cout, None, bias.cuda())
    srcs = [_dev_nhwc(x, 4 * i) for i, x in enumerate(xs)]                 # a different pixel stride per source
    buf = torch.full((B, Ho, Wo, cout + 4), float("nan"), device="cuda")
    out = buf[..., :cout]
    kw_ = dict(kh=kh, kw=kw, stride=stride, pad_yx=pad_yx, tile=tile, split_bf16=False)
    if S == 1:
        las = [ops.conv2d_launch(srcs, wp, sc, sh, out, cout=cout, **kw_)]
    else:
        ws = torch.full((S, B * Ho * Wo, ldw), float("nan"), device="cuda")
        las = [ops.conv2d_launch(srcs, wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw, ksplit=S, **kw_),
               ops.splitk_reduce_launch(ws, sc, sh, out, cout=cout)]
    got = _twice(las, lambda: buf.cpu())
    assert torch.isnan(got[..., cout:]).all(), "stored past the channels the launch was given"
    return las[0].kernel, got[..., :cout].permute(0, 3, 1, 2).double(), ref


# (id, source channels, cout, kh, kw, stride, (py, px), H, W): B = 1 throughout; 9 x 11 = 99 output pixels at stride 1 (one full and
# one ragged 64-row tile, one ragged 128-row tile), 5 x 6 = 30 at stride 2
CONV = [
    ("1x1-k1", (16,), 40, 1, 1, 1, (0, 0), 9, 11),
    ("1x1-k2", (32,), 40, 1, 1, 1, (0, 0), 9, 11),
    ("1x1-k3", (48,), 100, 1, 1, 1, (0, 0), 9, 11),
    ("1x1-k5", (80,), 40, 1, 1, 1, (0, 0), 9, 11),
    ("3x3s2-c16", (16,), 40, 3, 3, 2, (1, 1), 9, 11),
    ("3x3s2-c48", (48,), 100, 3, 3, 2, (1, 1), 9, 11),
    ("3x3s1-c16", (16,), 40, 3, 3, 1, (1, 1), 9, 11),
    ("root-16+32", (16, 32), 40, 1, 1, 1, (0, 0), 9, 11),
    ("root-16+32+48", (16, 32, 48), 100, 1, 1, 1, (0, 0), 9, 11),
]


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("case", CONV, ids=[c[0] for c in CONV])
def test_generic_conv_exact(case, tile):
    cid, srcC, cout, kh, kw, stride, pad, H, W = case
    kernel, got, ref = _conv_exact(100 + CONV.index(case), srcC, cout, kh, kw, stride, pad, 1, H, W, tile)
    assert kernel == TILES[tile]
    assert float(ref.abs().max()) < 2.0 ** 24
    assert torch.equal(got, ref), "first difference at %s" % (lo.first_unequal(got, ref),)


# 9 k-steps: S = 2 -> [0, 4) and [4, 9) (an even and an odd count; with three steps per tap the second starts inside tap 1);
# S = 3 -> three times three steps
SPLIT = [("3x3-c16", (16,), 3, 3, (1, 1)), ("1x3-c48", (48,), 1, 3, (0, 1))]


@pytest.mark.parametrize("S", (2, 3))
@pytest.mark.parametrize("case", SPLIT, ids=[c[0] for c in SPLIT])
def test_generic_conv_split_k_exact(case, S):
    cid, srcC, kh, kw, pad = case
    assert sum(srcC) * kh * kw // 16 == 9
    kernel, got, ref = _conv_exact(200 + 10 * SPLIT.index(case) + S, srcC, 40, kh, kw, 1, pad, 1, 9, 11, 64064, S=S)
    assert kernel == IG64
    assert torch.equal(got, ref), "first difference at %s" % (lo.first_unequal(got, ref),)


def test_generic_conv_group_exact():
    """two members of different K in one launch: 3x3 / stride 2 on 48 channels (27 k-steps, border taps) and 1x1 on 32 channels (2)"""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(300)
    spec = [(48, 40, 3, 2, 1), (32, 64, 1, 1, 0)]                          # cin, cout, k, stride, pad
    B, H, W = 1, 9, 11
    members, refs, views = [], [], []
    shapes = [((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1) for _, _, k, s, p in spec]
    whole = torch.full((sum(B * ho * wo * (co + 4) for (ho, wo), (_, co, _, _, _) in zip(shapes, spec)),), float("nan"), device="cuda")
    at = 0
    for (ci, co, k, s, p), (ho, wo) in zip(spec, shapes):
        x, w, bias = _ints(g, (B, ci, H, W), -3, 3), _ints(g, (co, ci, k, k), -2, 2), _ints(g, (co,), -5, 5)
        refs.append(F.conv2d(x.double(), w.double(), bias.double(), stride=s, padding=p))
        n = B * ho * wo * (co + 4)
        buf = whole[at:at + n].view(B, ho, wo, co + 4)
        at += n
        views.append(buf)
        sc, sh = ops.fold_bn(co, None, bias.cuda())
        members.append(dict(x=_dev_nhwc(x), wp=ops.pack_conv_weight(w.cuda()), scale=sc, shift=sh, out=buf[..., :co], cout=co, k=k, stride=s,
                            pad=p, act=ops.ACT_NONE, res=None))
    la = ops.conv2d_group_launch(members, whole)
    got = _twice([la], lambda: whole.cpu())
    assert la.kernel == "igemm_conv_group_kernel"
    at = 0
    for (ci, co, k, s, p), (ho, wo), ref in zip(spec, shapes, refs):
        n = B * ho * wo * (co + 4)
        o = got[at:at + n].view(B, ho, wo, co + 4)
        at += n
        assert torch.isnan(o[..., co:]).all(), "stored past the channels the member was given"
        o = o[..., :co].permute(0, 3, 1, 2).double()
        assert torch.equal(o, ref), "member %dx%d/%d: first difference at %s" % (k, k, ci, lo.first_unequal(o, ref))


# ---- DCNv2: exact answers -------------------------------------------------------------------------------------------------------------
DCN_TILES = {64064: ("dcn_igemm_kernel<64, 64, 2, 2, 32>", 40), 64128: ("dcn_igemm_kernel<64, 128, 2, 2, 32>", 128)}      # kernel, cout


@functools.lru_cache(maxsize=None)
def _dcn_data(C, cout):
    """integer input and weights, offsets on the half-integer grid in [-4, 4], masks in {0, 1/2, 1}; B = 1, 7 x 10 (70 pixels: one full
    and one ragged 64-row tile).  -> (x, w, bias, offset, mask, reference NCHW float64)"""
    from oracle import dcn as odcn
    g = torch.Generator().manual_seed(400 + C + cout)
    B, H, W = 1, 7, 10
    x, w, bias = _ints(g, (B, C, H, W), -3, 3), _ints(g, (cout, C, 3, 3), -2, 2), _ints(g, (cout,), -5, 5)
    off = _ints(g, (B, 18, H, W), -8, 8) * 0.5
    mask = _ints(g, (B, 9, H, W), 0, 2) * 0.5
    # samples leave the map on every side (and some stay inside): the validity rule and all four corner-zeroing rules are exercised
    ys = torch.arange(H).view(1, 1, H, 1) - 1 + (torch.arange(9) // 3).view(1, 9, 1, 1) + off[:, 0::2]
    xs_ = torch.arange(W).view(1, 1, 1, W) - 1 + (torch.arange(9) % 3).view(1, 9, 1, 1) + off[:, 1::2]
    assert (ys <= -1).any() and (ys >= H).any() and (xs_ <= -1).any() and (xs_ >= W).any()
    assert ((ys > -1) & (ys < 0)).any() and ((ys > H - 1) & (ys < H)).any() and ((xs_ > -1) & (xs_ < 0)).any() and ((xs_ > W - 1) & (xs_ < W)).any()
    ref = odcn.dcn_v2_forward_c(x.numpy(), w.numpy(), bias.numpy(), off.numpy(), mask.numpy())
    assert float(np.abs(ref).max()) < 2.0 ** 20                            # eighths of integers below 2^20: exact in float32
    return x, w, bias, off, mask, torch.from_numpy(ref).double()


@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("tile", sorted(DCN_TILES))
@pytest.mark.parametrize("C", (16, 32, 48))
def test_dcn_exact(C, tile, S):
    from centerpose_amd import ops
    kernel, cout = DCN_TILES[tile]
    x, w, bias, off, mask, ref = _dcn_data(C, cout)
    B, _, H, W = x.shape
    wp = ops.pack_conv_weight(w.cuda())
    ldw = wp.shape[0]
    assert ldw == (128 if tile == 64128 else 64)
    sc, sh = ops.fold_bn(cout, None, bias.cuda())
    om = torch.zeros(B, H, W, 32, device="cuda")
    om[..., :18] = off.permute(0, 2, 3, 1).cuda()
    om[..., 18:27] = mask.permute(0, 2, 3, 1).cuda()
    buf = torch.full((B, H, W, cout + 4), float("nan"), device="cuda")
    out = buf[..., :cout]
    if S == 1:
        las = [ops.dcn_v2_launch(_dev_nhwc(x, 4), om[..., :27], wp, sc, sh, out, cout=cout, om_sigmoid=False, tile=tile)]
    else:
        ws = torch.full((S, B * H * W, ldw), float("nan"), device="cuda")
        las = [ops.dcn_v2_launch(_dev_nhwc(x, 4), om[..., :27], wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw,
                                 om_sigmoid=False, tile=tile, ksplit=S),
               ops.splitk_reduce_launch(ws, sc, sh, out, cout=cout)]
    got = _twice(las, lambda: buf.cpu())
    assert las[0].kernel == kernel
    assert torch.isnan(got[..., cout:]).all(), "stored past the channels the launch was given"
    got = got[..., :cout].permute(0, 3, 1, 2).double()
    assert torch.equal(got, ref), "first difference at %s" % (lo.first_unequal(got, ref),)


# ---- F(2x4) convolution, single and grouped launch: float64 oracle at the existing `wino24` bound ------------------------------------
W24_SHAPES = {"48x48": (48, 48), "37x21": (37, 21)}
W24 = [(c, s, co, res) for c in (16, 32, 48) for s in W24_SHAPES for co in ((27, 27), (27, 32), (64, 64)) for res in (False, True)]


@functools.lru_cache(maxsize=None)
def _w24_case(cin, shape, cout, cpad, res):
    H, W = W24_SHAPES[shape]
    fast = cpad % 4 == 0
    row = L._r("diet-w24-c%d-%s-co%d-%d-%d" % (cin, shape, cout, cpad, res), "wino", "wino24", "conv3x3_wino24_kernel<%s>" % ("true" if fast else "false"),
               B=1, H=H, W=W, cin=cin, cout=cout, cpad=cpad, tile=24, res=res)
    g = torch.Generator().manual_seed(5000 + cin + 7 * H + cout + cpad + res)
    r = lambda *s: torch.randn(*s, generator=g)
    u01 = lambda n: torch.rand(n, generator=g)
    sd = lo.spread_bn({"b.weight": u01(cout) + 0.5, "b.bias": r(cout) * 0.1, "b.running_mean": r(cout) * 0.1, "b.running_var": u01(cout) + 0.5,
                       "c.weight": r(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5})
    return L.Case(row, row.p, sd, F.relu(r(1, cin, H, W)), F.relu(r(1, cout, H, W)) if res else None, None, H, W, cpad)


def _judge(case, out):
    with torch.no_grad():
        o64 = L.evaluate(case, torch.float64)
    w, fails = L.check(case, out, None, o64)
    print("\n%-32s worst err / (u A) %.3f (c = %.1f) at %s" % (case.row.id, w.ratio, lo.c_for(case.row.family, o64.K), w.loc))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cin,shape,co,res", W24, ids=["c%d-%s-co%d.%d%s" % (c, s, co[0], co[1], "-res" if res else "") for c, s, co, res in W24])
def test_wino24_conv_matches_fp64_reference(cin, shape, co, res):
    case = _w24_case(cin, shape, co[0], co[1], res)
    with torch.no_grad():
        launches, read = L.build_launches(case)
        out = _twice(launches, lambda: read()[1])
        assert read()[2], "stored past the channels the launch was given (NaN guard overwritten)"
    assert launches[0].kernel == case.row.kernel
    _judge(case, out)


@pytest.mark.parametrize("cpad", (27, 32), ids=["scalar-epilogue", "vector-epilogue"])
def test_wino24_group_matches_fp64_reference(cpad):
    """one grouped launch of three members with 1, 2 and 3 stages (16, 32, 48 input channels), ragged 37 x 21 map, residual on one"""
    from centerpose_amd import ops
    cases = [_w24_case(c, "37x21", 27, cpad, res) for c, res in ((48, True), (32, False), (16, False))]
    H, W = W24_SHAPES["37x21"]
    per = H * W * (cpad + 4 - cpad % 4)
    whole = torch.full((3 * per,), float("nan"), device="cuda")
    members = []
    for i, case in enumerate(cases):
        sd, cin = case.sd, case.p["cin"]
        buf = whole[i * per:(i + 1) * per].view(1, H, W, -1)
        wp = ops.pack_conv_weight(sd["c.weight"].cuda())
        sc, sh = ops.fold_bn(27, tuple(sd["b." + s].cuda() for s in ("weight", "bias", "running_mean", "running_var")))
        res = L._nhwc(case.res, cpad, -(-cpad // 4) * 4 + 4) if case.res is not None else None
        members.append(dict(x=L._nhwc(case.x), wp=wp, u24=ops.pack_wino24_weight(wp, cin, cpad), scale=sc, shift=sh, out=buf[..., :cpad], cout=cpad,
                            act=ops.ACT_RELU, res=res))
    la = ops.conv3x3_group_launch(members, whole)
    got = _twice([la], lambda: whole.cpu())
    assert la.kernel == "conv3x3_wino24_group_kernel<%s>" % ("true" if cpad % 4 == 0 else "false")
    for i, case in enumerate(cases):
        o = got[i * per:(i + 1) * per].view(1, H, W, -1)
        assert torch.isnan(o[..., cpad:]).all(), "member %d stored past its channels" % i
        assert (o[..., 27:cpad] == 0).all(), "member %d: padding channel not zero" % i
        _judge(case, o[..., :27].permute(0, 3, 1, 2).contiguous())


# ---- fused head kernels: all five instantiations, both forms ----------------------------------------------------------------------------
HEAD_SHAPES = {"32x32": (32, 32), "24x40": (24, 40)}
HEADS = [(s, n2) for s in HEAD_SHAPES for n2 in (1, 2, 17, 33, 34)]


@functools.lru_cache(maxsize=None)
def _head_case(shape, n2):
    H, W = HEAD_SHAPES[shape]
    hc = 128
    row = L._r("diet-head-%s-n%d" % (shape, n2), "head", "wino24", "head_wino24_kernel" + L._head_inst(n2), B=1, H=H, W=W, cin=64, hc=hc, cout=n2,
               sigmoid=False, wino24=True, res=False)
    g = torch.Generator().manual_seed(6000 + 100 * list(HEAD_SHAPES).index(shape) + n2)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"h.0.weight": r(hc, 64, 3, 3) * (2.0 / (9 * 64)) ** 0.5 * lo.spread_factors(hc).view(-1, 1, 1, 1), "h.0.bias": r(hc) * 0.1,
          "h.2.weight": r(n2, hc, 1, 1) * (2.0 / hc) ** 0.5 * lo.spread_factors(n2).view(-1, 1, 1, 1), "h.2.bias": r(n2) * 0.1}
    return L.Case(row, row.p, sd, r(1, 64, H, W), None, None, H, W, n2)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


@pytest.mark.parametrize("shape,n2", HEADS, ids=["%s-n%d" % h for h in HEADS])
def test_heads_both_forms_and_fp64_reference(shape, n2):
    case = _head_case(shape, n2)
    outs = {}
    for value in ("0", None):                                              # lock-step, then the default (staggered where it exists)
        with torch.no_grad():
            (la,), read = L.build_launches(case)
            with _env("CP_HEAD_STAGGER", value):
                outs[value] = _twice([la], lambda: read()[1])
            assert read()[2], "stored outside the output (NaN guard overwritten)"
        assert la.kernel == case.row.kernel
    assert torch.equal(outs["0"], outs[None]), "the two forms differ at %s" % (lo.first_unequal(outs[None], outs["0"]),)
    _judge(case, outs[None])
