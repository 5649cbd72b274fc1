"""The stage loop of `conv3x3_wino24_kernel` / `conv3x3_wino24_group_kernel` (w24_block): the U chunks stream from a scalar base that
stops at the last chunk, the halo patch is read through a buffer descriptor based at the block's first patch pixel -- a halo slot outside
the image has an offset past the descriptor's length and loads zero, so no tile selects zeros any more -- and the transform's operand
pairs are formed in front of the MFMA block.  What can go wrong: a U chunk too far or too few (whole terms), a halo slot that is not zero
(border values), a slot offset off by a row, a column, a channel quad or the block base (wrong pixels), a read outside the tensor.

Every case is one launch judged per element against the float64 evaluation of the same layer at the harness's own bound
(tests/launch_oracle.py / layer_oracle.py, family `wino24`; no tolerance of this file), runs twice and must give equal bits.  Inputs are
views whose surroundings (other channels of a wider buffer, the floats in front of a tensor placed at the end of its allocation) are NaN:
a read that leaves the view where the arithmetic uses it poisons the output.

* stage counts: C = 16, 32, 48, 80 (1, 2, 3, 5 stages: odd and even pairs, first and last U chunk, the stopped base);
* geometry: 17 x 19 (every tile a border tile, ragged on both edges), 49 x 49 (tile (1, 1) interior, tiles (2, .) and (., 2) ragged: the
  first patch pixel is clamped on none, one or both axes), 16 x 16 (one tile touching all four borders), each also on an input filled
  with a non-zero constant, where a missing halo zero is a wrong border value;
* channels out: 32, 40 (ragged last n-tile, lean epilogue), 27 (generic epilogue, `<false>`);
* epilogues: scale / shift only; residual + ReLU; the input a channel slice of a wider tensor (srcLd > C); every output is a slice
  (outLd > Cout, NaN guard behind it);
* allocation ends: the input placed at the very end of its allocation and a U buffer of exactly `cp_winograd24_weight_floats` floats;
* one group launch (cp_conv3x3_winograd24_group_f32) with two members of different C and map size;
* a map whose 18 patch rows span more than 2 GiB (2 x 32768 pixels, 1024 floats apart): the `*_far_kernel` instantiation, alone and as a
  member of a group launch;
* heads `<1, 0>`, `<2, 0>`, `<0, 1>` at 32 x 32 with CP_HEAD_STAGGER on and off: bit-equal to each other and within the bound.
"""
import contextlib
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import launch_oracle as L
import layer_oracle as lo

pytestmark = pytest.mark.gpu

SHAPES = {"17x19": (17, 19), "49x49": (49, 49), "16x16": (16, 16), "33x16": (33, 16), "2x32768": (2, 32768)}


@functools.lru_cache(maxsize=None)
def _case(cin, shape, cout, cpad, res, relu, const=False, B=2):
    H, W = SHAPES[shape]
    fast = cpad % 4 == 0
    row = L._r("w24loop-c%d-%s-co%d.%d-%d%d%d" % (cin, shape, cout, cpad, res, relu, const), "wino", "wino24",
               "conv3x3_wino24_kernel<%s>" % ("true" if fast else "false"), B=B, H=H, W=W, cin=cin, cout=cout, cpad=cpad, tile=24, res=res, relu=relu)
    g = torch.Generator().manual_seed(7000 + cin + 7 * H + 3 * W % 1000 + cout + cpad + 2 * res + relu)
    r = lambda *s: torch.randn(*s, generator=g)
    u01 = lambda n: torch.rand(n, generator=g)
    sd = lo.spread_bn({"b.weight": u01(cout) + 0.5, "b.bias": r(cout) * 0.1, "b.running_mean": r(cout) * 0.1, "b.running_var": u01(cout) + 0.5,
                       "c.weight": r(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5})
    x = torch.full((B, cin, H, W), 0.75) if const else F.relu(r(B, cin, H, W))
    return L.Case(row, row.p, sd, x, F.relu(r(B, cout, H, W)) if res else None, None, H, W, cpad)


def _src(x, mode):
    """logical NCHW CPU tensor -> device NHWC view.  "plain": its own dense tensor; "slice": channels [4, 4 + C) of a buffer C + 8 floats
    wide whose other channels are NaN; "end": the last floats of an allocation whose size is a multiple of 512 bytes, NaN in front"""
    B, C, H, W = x.shape
    v = x.permute(0, 2, 3, 1).contiguous().cuda()
    if mode == "plain":
        return v
    if mode == "slice":
        buf = torch.full((B, H, W, C + 8), float("nan"), device="cuda")
        buf[..., 4:4 + C] = v
        return buf[..., 4:4 + C]
    n = v.numel()
    pre = 128 + (-n) % 128
    flat = torch.full((pre + n,), float("nan"), device="cuda")
    assert flat.untyped_storage().nbytes() == (pre + n) * 4 and (pre + n) * 4 % 512 == 0
    flat[pre:] = v.reshape(-1)
    return flat[pre:].view(B, H, W, C)


def _member(case, src="plain"):
    """-> (keyword set of the launch, NaN-guarded buffer, its view) for one convolution of `case`"""
    from centerpose_amd import _lib, ops
    p, sd, cp = case.p, case.sd, case.cpad
    wp = ops.pack_conv_weight(sd["c.weight"].cuda())
    u = ops.pack_wino24_weight(wp, p["cin"], cp)
    L_ = _lib.lib()
    L_.cp_winograd24_weight_floats.restype = ctypes.c_size_t
    assert u.numel() == L_.cp_winograd24_weight_floats(p["cin"], cp) == 24 * (-(-cp // 32)) * 32 * p["cin"]      # not one float more
    sc, sh = ops.fold_bn(p["cout"], tuple(sd["b." + s].cuda() for s in ("weight", "bias", "running_mean", "running_var")))
    buf, out = L._guarded(p["B"], p["H"], p["W"], cp)
    res = L._nhwc(case.res, cp, -(-cp // 4) * 4 + 4) if case.res is not None else None
    return dict(x=_src(case.x, src), wp=wp, u24=u, scale=sc, shift=sh, out=out, cout=cp, act=ops.ACT_RELU if p["relu"] else ops.ACT_NONE, res=res), buf, out


def _twice(launch, read):
    launch.run()
    torch.cuda.synchronize()
    first = read()
    launch.run()
    torch.cuda.synchronize()
    second = read()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(first), bits(second)), "a second run gives other bits at %s" % (lo.first_unequal(bits(first), bits(second)),)
    return first


def _judge(case, out):
    with torch.no_grad():
        o64 = L.evaluate(case, torch.float64)
    w, fails = L.check(case, out, None, o64)
    print("\n%-40s worst err / (u A) %.3f (c = %.1f) at %s" % (case.row.id, w.ratio, lo.c_for(case.row.family, o64.K), w.loc))
    assert not fails, "\n".join(fails)


def _run(case, src="plain", kernel=None):
    from centerpose_amd import ops
    p, cp, co = case.p, case.cpad, case.p["cout"]
    with torch.no_grad():
        m, buf, out = _member(case, src)
        la = ops.conv2d_launch([m["x"]], m["wp"], m["scale"], m["shift"], out, kh=3, kw=3, stride=1, pad=1, cout=cp, act=m["act"], res=m["res"],
                               wino=m["u24"], tile=ops.WINO24, split_bf16=False)
        got = _twice(la, lambda: buf.cpu())
    assert la.kernel == (kernel or case.row.kernel)
    assert torch.isnan(got[..., cp:]).all(), "stored past the channels the launch was given (NaN guard overwritten)"
    assert (got[..., co:cp] == 0).all(), "padding channel not zero"
    _judge(case, got[..., :co].permute(0, 3, 1, 2).contiguous())


@pytest.mark.parametrize("cin", (16, 32, 48, 80))
def test_stage_counts(cin):
    _run(_case(cin, "17x19", 32, 32, True, True))


@pytest.mark.parametrize("const", (False, True), ids=("random", "constant"))
@pytest.mark.parametrize("shape", ("17x19", "49x49", "16x16"))
def test_geometry(shape, const):
    _run(_case(32, shape, 40, 40, False, False, const))


@pytest.mark.parametrize("co", ((32, 32), (40, 40), (27, 27)), ids=("co32", "co40-ragged-ntile", "co27-generic"))
@pytest.mark.parametrize("res,relu", ((False, False), (True, True)), ids=("scale-shift", "res-relu"))
def test_channels_out_and_epilogues(co, res, relu):
    _run(_case(48, "49x49", co[0], co[1], res, relu))


@pytest.mark.parametrize("shape", ("17x19", "49x49"))
@pytest.mark.parametrize("src", ("slice", "end"))
def test_input_slice_and_allocation_end(src, shape):
    """srcLd > C with NaN in the neighbouring channels; the input at the very end of its allocation (NaN in front) with a U buffer of exactly
    cp_winograd24_weight_floats floats (`_member` asserts the size)"""
    _run(_case(48, shape, 40, 40, True, True), src)


def test_group_launch_two_members():
    """one grouped launch: 48 channels on 17 x 19 with a residual, 16 channels on 33 x 16 without"""
    from centerpose_amd import ops
    cases = [_case(48, "17x19", 40, 40, True, True), _case(16, "33x16", 32, 32, False, True)]
    with torch.no_grad():
        per = [c.p["B"] * c.p["H"] * c.p["W"] * (c.cpad + 4) for c in cases]
        whole = torch.full((sum(per),), float("nan"), device="cuda")
        members, at = [], 0
        for c, n, src in zip(cases, per, ("slice", "end")):
            m, _, _ = _member(c, src)
            m["out"] = whole[at:at + n].view(c.p["B"], c.p["H"], c.p["W"], c.cpad + 4)[..., :c.cpad]
            members.append(m)
            at += n
        la = ops.conv3x3_group_launch(members, whole)
        got = _twice(la, lambda: whole.cpu())
    assert la.kernel == "conv3x3_wino24_group_kernel<true>"
    at = 0
    for c, n in zip(cases, per):
        o = got[at:at + n].view(c.p["B"], c.p["H"], c.p["W"], c.cpad + 4)
        at += n
        assert torch.isnan(o[..., c.cpad:]).all(), "%s stored past its channels" % c.row.id
        _judge(c, o[..., :c.p["cout"]].permute(0, 3, 1, 2).contiguous())


def _far_member():
    """(17 W + 17) ld + C floats of patch span > 2 GiB: W = 32768 pixels 1024 floats apart (the input is a 16-channel slice), two rows"""
    H, W = SHAPES["2x32768"]
    assert ((17 * W + 17) * 1024 + 16) * 4 > 2 ** 31
    case = _case(16, "2x32768", 32, 32, False, True, B=1)
    m, buf, out = _member(case)
    wide = torch.full((1, H, W, 1024), float("nan"), device="cuda")
    wide[..., 4:20] = m["x"]
    m["x"] = wide[..., 4:20]
    return case, m, buf, out


def test_far_tensor_takes_the_64_bit_instantiation():
    from centerpose_amd import ops
    with torch.no_grad():
        case, m, buf, out = _far_member()
        cp = case.cpad
        la = ops.conv2d_launch([m["x"]], m["wp"], m["scale"], m["shift"], out, kh=3, kw=3, stride=1, pad=1, cout=cp, act=m["act"], res=None,
                               wino=m["u24"], tile=ops.WINO24, split_bf16=False)
        got = _twice(la, lambda: buf.cpu())
    assert la.kernel == "conv3x3_wino24_far_kernel<true>"
    assert torch.isnan(got[..., cp:]).all(), "stored past the channels the launch was given"
    _judge(case, got[..., :cp].permute(0, 3, 1, 2).contiguous())


def test_group_with_a_far_member():
    """the far tensor and a small map in one grouped launch: the whole group takes the 64-bit instantiation"""
    from centerpose_amd import ops
    with torch.no_grad():
        far, mf, _, _ = _far_member()
        small = _case(48, "17x19", 40, 40, True, True)
        ms, _, _ = _member(small, "slice")
        cases, members = [far, small], [mf, ms]
        per = [c.p["B"] * c.p["H"] * c.p["W"] * (c.cpad + 4) for c in cases]
        whole = torch.full((sum(per),), float("nan"), device="cuda")
        at = 0
        for c, m, n in zip(cases, members, per):
            m["out"] = whole[at:at + n].view(c.p["B"], c.p["H"], c.p["W"], c.cpad + 4)[..., :c.cpad]
            at += n
        la = ops.conv3x3_group_launch(members, whole)
        got = _twice(la, lambda: whole.cpu())
    assert la.kernel == "conv3x3_wino24_group_far_kernel<true>"
    at = 0
    for c, n in zip(cases, per):
        o = got[at:at + n].view(c.p["B"], c.p["H"], c.p["W"], c.cpad + 4)
        at += n
        assert torch.isnan(o[..., c.cpad:]).all(), "%s stored past its channels" % c.row.id
        _judge(c, o[..., :c.p["cout"]].permute(0, 3, 1, 2).contiguous())


# ---- heads: the three instantiations of the timed network, both forms ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_case(n2):
    H, W, hc = 32, 32, 128
    row = L._r("w24loop-head-n%d" % n2, "head", "wino24", "head_wino24_kernel" + L._head_inst(n2), B=1, H=H, W=W, cin=64, hc=hc, cout=n2,
               sigmoid=False, wino24=True, res=False)
    g = torch.Generator().manual_seed(7500 + n2)
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


@pytest.mark.parametrize("n2", (1, 2, 17), ids=("<1, 0>", "<2, 0>", "<0, 1>"))
def test_heads_both_forms(n2):
    case = _head_case(n2)
    outs = {}
    for value in ("0", None):                                              # lock-step, then the default (staggered where it exists)
        with torch.no_grad():
            (la,), read = L.build_launches(case)
            with _env("CP_HEAD_STAGGER", value):
                outs[value] = _twice(la, lambda: read()[1])
            assert read()[2], "stored outside the output (NaN guard overwritten)"
        assert la.kernel == case.row.kernel
    assert torch.equal(outs["0"], outs[None]), "the two forms differ at %s" % (lo.first_unequal(outs[None], outs["0"]),)
    _judge(case, outs[None])
