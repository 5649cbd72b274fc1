"""GPU: fused conv / DCNv2 / pooling / upsampling kernels (through the C ABI) against plain
torch-CPU fp32 references of the same op and the scalar C DCN oracle.
Tolerance: fp32 in / fp32 accumulate on MFMA -> |err| <= 2e-4 * max|ref| (summation order only).
The per-element judgement of the variants forced here through `tile=` / `ksplit=` / `wino24=` (|out - ref64| <= c u A on post-ReLU data
with a per-channel scale spread) lives in tests/test_variant_parity_hip.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from cases import _dcn_case, _dcn_mask_logits

pytestmark = pytest.mark.gpu


def _close(out, ref, tol=2e-4):
    out, ref = out.detach().cpu().double(), ref.detach().cpu().double()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = (out - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-6)
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _rand_bn(g, c):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1,
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5)


def _ref_bn(y, bn):
    gm, b, m, v = bn
    return F.batch_norm(y, m, v, gm, b, False, 0.0, 1e-5)


@pytest.mark.parametrize("cin,cout,k,s,p,hw,tile", [
    (32, 64, 3, 1, 1, (20, 28), 0), (16, 32, 3, 2, 1, (33, 17), 0), (64, 128, 1, 1, 0, (9, 9), 0),
    (16, 16, 3, 1, 1, (40, 24), 256016), (32, 32, 3, 1, 1, (16, 16), 128032), (64, 64, 3, 1, 1, (16, 16), 128064),
    (64, 64, 3, 1, 1, (16, 16), 64064), (48, 128, 3, 1, 1, (24, 24), 128128), (128, 27, 3, 1, 1, (16, 16), 0),
    (256, 512, 3, 2, 1, (8, 8), 0), (32, 48, 3, 1, 1, (12, 12), 256016),
])
def test_conv_bn_relu_residual(cin, cout, k, s, p, hw, tile):
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cin * 131 + cout)
    B, (H, W) = 3, hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bn = _rand_bn(g, cout)
    ref = _ref_bn(F.conv2d(x, w, None, s, p), bn)
    res = torch.randn(ref.shape, generator=g)
    ref = F.relu(ref + res)
    wp = ops.pack_conv_weight(w.cuda())
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    Ho, Wo = ref.shape[2:]
    out = torch.empty(B, Ho, Wo, cout, device="cuda")
    ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=k, kw=k, stride=s, pad=p, cout=cout, act=ops.ACT_RELU,
               res=_nhwc(res), tile=tile)
    _close(out.permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("cin,cout,k,s,p,hw,bn_tile", [
    (32, 64, 3, 1, 1, (20, 28), 64), (64, 128, 1, 1, 0, (9, 9), 128), (64, 128, 1, 1, 0, (9, 9), 64), (256, 512, 3, 2, 1, (8, 8), 128),
    (48, 128, 3, 1, 1, (24, 24), 128), (128, 64, 1, 1, 0, (33, 17), 64), (1024, 256, 1, 1, 0, (7, 5), 128), (16, 64, 3, 2, 1, (33, 17), 64),
    (64, 128, 1, 1, 0, (9, 9), "64x128"), (256, 512, 3, 2, 1, (8, 8), "64x64"), (1024, 256, 1, 1, 0, (7, 5), "64x128"), (32, 64, 3, 1, 1, (20, 28), "64x64"),
    (48, 128, 3, 1, 1, (24, 24), "64x64"),
])
def test_conv_split_bf16_matches_f32_kernel_tolerance(cin, cout, k, s, p, hw, bn_tile):
    """The OPT-IN split-bf16 kernel (conv_igemm_bf16x3.hip: three bf16 terms per fp32 operand, six bf16 MFMAs, fp32 accumulate) on the
    cases of test_conv_bn_relu_residual, at the SAME tolerance as the f32-MFMA kernel, and within 2x of that kernel's own error
    against an fp64 reference (ragged M / edge tiles, stride 2, residual, 1x1 and 3x3, both N tiles)."""
    from centerpose_amd import _lib, ops
    g = torch.Generator().manual_seed(cin * 131 + cout)
    B, (H, W) = 3, hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bn = _rand_bn(g, cout)
    res = None
    ref64 = F.conv2d(x.double(), w.double(), None, s, p)
    gm, b, m, v = (t.double() for t in bn)
    ref64 = (ref64 - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + 1e-5) * gm[None, :, None, None] + b[None, :, None, None]
    res = torch.randn(ref64.shape, generator=g)
    ref64 = F.relu(ref64 + res.double())
    wp = ops.pack_conv_weight(w.cuda())
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    Ho, Wo = ref64.shape[2:]
    outs = {}
    for mode in ("f32", "bf16x3"):
        out = torch.full((B, Ho, Wo, cout), float("nan"), device="cuda")
        if mode == "f32":
            ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=k, kw=k, stride=s, pad=p, cout=cout, act=ops.ACT_RELU, res=_nhwc(res), tile=64064)
        else:
            import os
            os.environ["CP_SPLIT_BF16_TILE"] = str(bn_tile)
            try:
                ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=k, kw=k, stride=s, pad=p, cout=cout, act=ops.ACT_RELU, res=_nhwc(res), split_bf16=True)
            finally:
                del os.environ["CP_SPLIT_BF16_TILE"]
            want = "igemm_bf16x3_kernel<%s>" % (bn_tile.replace("x", ", ") if isinstance(bn_tile, str) else "128, %d" % bn_tile)
            assert _lib.lib().cp_last_kernel().decode() == want
        outs[mode] = out.permute(0, 3, 1, 2)
        _close(outs[mode], ref64.float())
    e32 = (outs["f32"].cpu().double() - ref64).abs().max().item()
    e16 = (outs["bf16x3"].cpu().double() - ref64).abs().max().item()
    print("%d->%d k%d s%d %s: max err vs fp64  f32 MFMA %.2e   split-bf16 %.2e" % (cin, cout, k, s, hw, e32, e16))
    assert e16 <= 2.0 * e32 + 1e-7


@pytest.mark.parametrize("cin,cout,B,hw,res,act", [(64, 256, 3, (33, 17), True, 1), (64, 64, 2, (16, 16), False, 0), (64, 512, 2, (20, 13), True, 0),
                                                   (64, 128, 1, (9, 130), False, 1), (64, 40, 2, (12, 12), True, 1)])
def test_conv_pointwise_kernel_bit_identical_to_generic(cin, cout, B, hw, res, act):
    """conv_pointwise.hip (round 6): the short-K 1x1 kernel that requests its whole A / weight / residual tiles up front (the HBM-bound
    Bottleneck conv3 / downsample layers, msra_resnet.py:82-102) -- forced with tile code 1 -- against the generic implicit-GEMM kernel
    (tile 64064) on the same inputs: BIT-IDENTICAL (same accumulation order, same epilogue expression), and both against torch;
    ragged M (edge tiles), output channels that are not a multiple of the 64-wide tile, with / without residual and ReLU.  An
    ineligible shape asked for by code raises instead of falling back."""
    from centerpose_amd import _lib, ops
    g = torch.Generator().manual_seed(cin + cout)
    H, W = hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bn = _rand_bn(g, cout)
    r = torch.randn(B, cout, H, W, generator=g) if res else None
    ref = _ref_bn(F.conv2d(x, w), bn)
    if res:
        ref = ref + r
    if act:
        ref = F.relu(ref)
    wp = ops.pack_conv_weight(w.cuda())
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    outs = {}
    for tile in (1, 64064):
        buf = torch.full((B, H, W, cout + 8), float("nan"), device="cuda")
        out = buf[..., :cout]
        la = ops.conv2d_launch([_nhwc(x)], wp, sc, sh, out, kh=1, kw=1, cout=cout, act=act, res=_nhwc(r) if res else None, tile=tile)
        la.run()
        assert la.kernel.startswith("pw_conv_kernel" if tile == 1 else "igemm_conv_kernel"), la.kernel
        assert torch.isnan(buf[..., cout:]).all()
        outs[tile] = out.clone()
        _close(out.permute(0, 3, 1, 2), ref)
    assert torch.equal(outs[1], outs[64064])
    with pytest.raises(_lib.CenterposeHipError):                   # 3x3: not this kernel's shape
        w3 = ops.pack_conv_weight(torch.randn(64, cin, 3, 3).cuda())
        ops.conv2d([_nhwc(x)], w3, *ops.fold_bn(64, None, torch.zeros(64).cuda()), torch.empty(B, H, W, 64, device="cuda"), kh=3, kw=3, pad=1, cout=64, tile=1)
    with pytest.raises(_lib.CenterposeHipError):                   # K = 128: measured, did not pay, not built in
        x2 = torch.randn(B, H, W, 128, device="cuda")
        ops.conv2d([x2], ops.pack_conv_weight(torch.randn(64, 128, 1, 1).cuda()), *ops.fold_bn(64, None, torch.zeros(64).cuda()),
                   torch.empty(B, H, W, 64, device="cuda"), kh=1, kw=1, cout=64, tile=1)
    auto = ops.conv2d_launch([_nhwc(x)], wp, sc, sh, torch.empty(B, H, W, cout, device="cuda"), kh=1, kw=1, cout=cout, act=act, res=_nhwc(r) if res else None)
    auto.run()
    assert auto.kernel.startswith("pw_conv_kernel")               # the default rule takes it for every eligible launch


@pytest.mark.parametrize("xs,ws", [(1e30, 1e-30), (1e-30, 1e30), (3e18, 3e18), (1e-19, 1e-19)])
def test_conv_split_bf16_magnitude_range(xs, ws):
    """the split-bf16 kernel's DOMAIN is finite operands below 2^127 (conv_igemm_bf16x3.hip header): across 60 binades of
    operand magnitude -- products up to 1e37, down to 1e-38 -- it stays at the f32 kernel's relative error against an fp64 reference.
    (Non-finite operands are outside the domain: inf - bf16(inf) is NaN in the residual where the f32 kernel propagates inf.)"""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(11)
    B, C, Co, H, W = 2, 64, 64, 12, 12
    x = torch.randn(B, C, H, W, generator=g) * xs
    w = torch.randn(Co, C, 1, 1, generator=g) / 8 * ws
    ref = F.conv2d(x.double(), w.double())
    sc, sh = ops.fold_bn(Co, None, torch.zeros(Co).cuda())
    wp = ops.pack_conv_weight(w.cuda())
    err = {}
    for mode in ("f32", "bf16x3"):
        out = torch.empty(B, H, W, Co, device="cuda")
        ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=1, kw=1, cout=Co, **({"tile": 64064} if mode == "f32" else {"split_bf16": True}))
        got = out.permute(0, 3, 1, 2).cpu().double()
        assert torch.isfinite(got).all()
        err[mode] = ((got - ref).abs().max() / ref.abs().max()).item()
    print("scale %g x %g: relative error vs fp64  f32 MFMA %.2e  split-bf16 %.2e" % (xs, ws, err["f32"], err["bf16x3"]))
    assert err["bf16x3"] <= 2.0 * err["f32"] + 1e-7


def test_conv_split_bf16_concat_deconv_splitk_nchw():
    """The other producers / epilogues of the generic kernel through the split-bf16 kernel: concatenated sources with channel views
    (DLA Root), the fused sub-pixel deconvolution (nsub = 4), split-K + fixed-order reduction, and the NCHW head output."""
    from centerpose_amd import _lib, ops
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 10, 14
    xs = [torch.randn(B, c, H, W, generator=g) for c in (64, 32, 16, 48)]
    w = torch.randn(128, 160, 1, 1, generator=g) * 0.1
    bias = torch.randn(128, generator=g)
    ref = F.relu(F.conv2d(torch.cat(xs, 1), w, bias))
    wide = torch.randn(B, H, W, 96, generator=g).cuda()
    wide[..., 32:64] = _nhwc(xs[1])
    srcs = [_nhwc(xs[0]), wide[..., 32:64], _nhwc(xs[2]), _nhwc(xs[3])]
    sc, sh = ops.fold_bn(128, None, bias.cuda())
    out = torch.empty(B, H, W, 128, device="cuda")
    ops.conv2d(srcs, ops.pack_conv_weight(w.cuda()), sc, sh, out, kh=1, kw=1, cout=128, act=ops.ACT_RELU, split_bf16=True)
    assert _lib.lib().cp_last_kernel().decode().startswith("igemm_bf16x3_kernel")
    _close(out.permute(0, 3, 1, 2), ref)
    # fused sub-pixel deconvolution
    C, Co, H, W = 32, 64, 9, 11
    x = torch.randn(B, C, H, W, generator=g)
    wd = torch.randn(C, Co, 4, 4, generator=g) * 0.1
    bn = _rand_bn(g, Co)
    ref = F.relu(_ref_bn(F.conv_transpose2d(x, wd, None, 2, 1), bn))
    sc, sh = ops.fold_bn(Co, tuple(t.cuda() for t in bn))
    out4 = torch.full((B, 2 * H, 2 * W, Co), float("nan"), device="cuda")
    wp4 = torch.cat([ops.pack_deconv4_subpixel(wd.cuda(), py_, px_) for py_ in range(2) for px_ in range(2)], 0).contiguous()
    ops.conv2d([_nhwc(x)], wp4, sc, sh, out4, kh=2, kw=2, stride=1, pad=0, pad_yx=(1, 1), cout=Co, act=ops.ACT_RELU, Ho=H, Wo=W,
               out_scatter=(2, 2, 0, 0), nsub=4, split_bf16=True)
    assert _lib.lib().cp_last_kernel().decode().startswith("igemm_bf16x3_kernel")
    _close(out4.permute(0, 3, 1, 2), ref)
    # split-K (raw partial sums) + reduction
    cin, cout, S = 512, 128, 3
    x = torch.randn(B, cin, 6, 7, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bn = _rand_bn(g, cout)
    ref = F.relu(_ref_bn(F.conv2d(x, w, None, 2, 1), bn))
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    wp = ops.pack_conv_weight(w.cuda())
    M, ldw = B * ref.shape[2] * ref.shape[3], wp.shape[0]
    ws = torch.full((S, M, ldw), float("nan"), device="cuda")
    ops.conv2d([_nhwc(x)], wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, kh=3, kw=3, stride=2, pad=1, cout=ldw,
               ksplit=S, split_bf16=True)
    assert _lib.lib().cp_last_kernel().decode().startswith("igemm_bf16x3_kernel")
    out = torch.empty(B, ref.shape[2], ref.shape[3], cout, device="cuda")
    ops.splitk_reduce_launch(ws, sc, sh, out, cout=cout, act=ops.ACT_RELU).run()
    _close(out.permute(0, 3, 1, 2), ref)
    # NCHW output + sigmoid (ldw = 64 for 34 outputs)
    x = torch.randn(2, 64, 12, 20, generator=g)
    w = torch.randn(34, 64, 1, 1, generator=g) * 0.2
    b = torch.randn(34, generator=g)
    ref = torch.sigmoid(F.conv2d(x, w, b))
    sc, sh = ops.fold_bn(34, None, b.cuda())
    out = torch.empty(2, 34, 12, 20, device="cuda")
    ops.conv2d([_nhwc(x)], ops.pack_conv_weight(w.cuda()), sc, sh, out, kh=1, kw=1, cout=34, act=2, out_nchw=True, split_bf16=True)
    assert _lib.lib().cp_last_kernel().decode().startswith("igemm_bf16x3_kernel")
    _close(out, ref, 1e-5)


def test_conv2d_group_equals_single_launches():
    """cp_conv2d_group_f32 (HRNet's fuse layers as ONE launch, pose_higher_hrnet.py:169-212): eight independent convs of mixed kind --
    1x1 and stride-2 3x3, 16..256 input channels, 32..256 outputs (padded to the shared 64-wide tile), ragged maps, ReLU or not --
    must give the SAME BITS as the eight single launches of the 64 x 64 tile, and agree with torch-CPU."""
    from centerpose_amd import _lib, ops
    g = torch.Generator().manual_seed(11)
    B = 2
    cases = [(32, 64, 3, 2, 1, (24, 20), True), (64, 32, 1, 1, 0, (12, 10), False), (128, 32, 1, 1, 0, (6, 5), False), (256, 64, 1, 1, 0, (3, 3), False),
             (32, 32, 3, 2, 1, (24, 20), True), (64, 128, 3, 2, 1, (12, 10), False), (128, 256, 3, 2, 1, (7, 5), False), (16, 48, 1, 1, 0, (9, 11), True)]
    recs, refs, singles = [], [], []
    sizes = []
    for cin, cout, k, st, pd, (H, W), relu in cases:
        Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        sizes.append(B * Ho * Wo * ops.round_up(cout, 16))
    whole = torch.full((sum(sizes),), float("nan"), device="cuda")
    off = 0
    for (cin, cout, k, st, pd, (H, W), relu), n in zip(cases, sizes):
        x = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        bn = _rand_bn(g, cout)
        ref = _ref_bn(F.conv2d(x, w, None, st, pd), bn)
        refs.append(F.relu(ref) if relu else ref)
        Ho, Wo = ref.shape[2:]
        cp = ops.round_up(cout, 16)
        wp = ops.pack_conv_weight(w.cuda())
        sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
        ldw = ops.round_up(wp.shape[0], 64)
        wp, sc, sh = ops.pad_rows(wp, ldw), ops.pad_vec(sc, ldw), ops.pad_vec(sh, ldw)
        out = whole[off:off + n].view(B, Ho, Wo, cp)
        off += n
        recs.append(dict(x=_nhwc(x), wp=wp, scale=sc, shift=sh, out=out, cout=cp, k=k, stride=st, pad=pd, act=ops.ACT_RELU if relu else ops.ACT_NONE))
        one = torch.full((B, Ho, Wo, cp), float("nan"), device="cuda")
        ops.conv2d([recs[-1]["x"]], wp, sc, sh, one, kh=k, kw=k, stride=st, pad=pd, cout=cp, act=recs[-1]["act"], tile=64064, split_bf16=False)
        singles.append(one)
    la = ops.conv2d_group_launch(recs, whole)
    la.run()
    assert la.kernel == "igemm_conv_group_kernel"
    for r, one, ref, (cin, cout, *_rest) in zip(recs, singles, refs, cases):
        assert torch.equal(r["out"], one), "%d->%d: grouped launch differs from the single launch" % (cin, cout)
        assert (r["out"][..., cout:] == 0).all()                                  # padding channels are written as exact zeros
        _close(r["out"][..., :cout].permute(0, 3, 1, 2), ref)
    with pytest.raises(Exception):
        ops.conv2d_group_launch(recs + recs[:1], whole)                            # nine members


def test_conv_concat_sources_and_channel_views():
    """Root: cat -> 1x1 conv (pose_dla_dcn.py:155-163) without materialising the cat; sources may be
    channel slices of wider tensors (pixel stride > C)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 10, 14
    xs = [torch.randn(B, c, H, W, generator=g) for c in (64, 32, 16, 48)]
    w = torch.randn(80, 160, 1, 1, generator=g) * 0.1
    bias = torch.randn(80, generator=g)
    ref = F.relu(F.conv2d(torch.cat(xs, 1), w, bias))
    wide = torch.randn(B, H, W, 96, generator=g).cuda()          # source 1 lives inside a wider buffer
    wide[..., 32:64] = _nhwc(xs[1])
    srcs = [_nhwc(xs[0]), wide[..., 32:64], _nhwc(xs[2]), _nhwc(xs[3])]
    sc, sh = ops.fold_bn(80, None, bias.cuda())
    out = torch.empty(B, H, W, 80, device="cuda")
    ops.conv2d(srcs, ops.pack_conv_weight(w.cuda()), sc, sh, out, kh=1, kw=1, cout=80, act=ops.ACT_RELU)
    _close(out.permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("cout,k,s,p,hw,tile", [(16, 7, 1, 3, (40, 36), 0), (64, 7, 2, 3, (37, 41), 0),
                                                (64, 3, 2, 1, (32, 32), 0), (32, 7, 1, 3, (24, 24), 0), (64, 3, 2, 1, (37, 52), 0),
                                                (64, 3, 2, 1, (256, 384), 0), (64, 3, 2, 1, (21, 30), 0), (64, 3, 2, 1, (32, 32), 128064)])
def test_stem_nchw_input(cout, k, s, p, hw, tile):
    """network input is NCHW float32 with 3 channels (base_detector.py:53-58).  3x3 / stride 2 / 64 outputs with whole float4 quads per row
    (HRNet conv1, pose_higher_hrnet.py:283-285) goes to the persistent stem kernel; everything else to the scalar-gather producer."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cout + k)
    x = torch.randn(2, 3, *hw, generator=g)
    w = torch.randn(cout, 3, k, k, generator=g) * 0.1
    bn = _rand_bn(g, cout)
    ref = F.relu(_ref_bn(F.conv2d(x, w, None, s, p), bn))
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    out = torch.empty(2, ref.shape[2], ref.shape[3], cout, device="cuda")
    ops.conv2d([x.cuda()], ops.pack_conv_weight(w.cuda(), stem=True), sc, sh, out, kh=k, kw=k, stride=s, pad=p,
               cout=cout, act=ops.ACT_RELU, in_nchw=True, tile=tile)
    from centerpose_amd import _lib
    pers = (cout, k, s, p) == (64, 3, 2, 1) and hw[1] % 4 == 0 and tile == 0
    assert _lib.lib().cp_last_kernel().decode().startswith("stem7x7_c16_kernel<64, 2, 3>" if pers else "igemm_conv_kernel")
    _close(out.permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("cout,act", [(1, 2), (2, 0), (34, 0), (17, 2)])
def test_head_1x1_nchw_output(cout, act):
    """KeypointHead final 1x1 conv (+bias) writing the reference's NCHW output, hm/hm_hp sigmoided
    (keypoint.py:14-42, multi_pose.py:35-37)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(2, 64, 12, 20, generator=g)
    w = torch.randn(cout, 64, 1, 1, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    ref = F.conv2d(x, w, b)
    if act == 2:
        ref = torch.sigmoid(ref)
    sc, sh = ops.fold_bn(cout, None, b.cuda())
    out = torch.empty(2, cout, 12, 20, device="cuda")
    ops.conv2d([_nhwc(x)], ops.pack_conv_weight(w.cuda()), sc, sh, out, kh=1, kw=1, cout=cout, act=act, out_nchw=True)
    _close(out, ref, 1e-5 if act == 2 else 2e-4)


def test_dense_deconv_as_subpixel_convs():
    """ConvTranspose2d(k4,s2,p1) (msra_resnet.py:168-193) == 4 interleaved 2x2 convs."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(3)
    B, C, Co, H, W = 2, 32, 64, 9, 11
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, Co, 4, 4, generator=g) * 0.1
    bn = _rand_bn(g, Co)
    ref = F.relu(_ref_bn(F.conv_transpose2d(x, w, None, 2, 1), bn))
    sc, sh = ops.fold_bn(Co, tuple(t.cuda() for t in bn))
    out = torch.empty(B, 2 * H, 2 * W, Co, device="cuda")
    xg = _nhwc(x)
    for py_ in range(2):
        for px_ in range(2):
            wp = ops.pack_deconv4_subpixel(w.cuda(), py_, px_)
            ops.conv2d([xg], wp, sc, sh, out, kh=2, kw=2, stride=1, pad=0, pad_yx=(1 - py_, 1 - px_), cout=Co,
                       act=ops.ACT_RELU, Ho=H, Wo=W, out_scatter=(2, 2, py_, px_))
    _close(out.permute(0, 3, 1, 2), ref)
    # the same four convolutions fused into one launch (nsub = 4): bit-identical to the four separate launches
    out4 = torch.full_like(out, float("nan"))
    wp4 = torch.cat([ops.pack_deconv4_subpixel(w.cuda(), py_, px_) for py_ in range(2) for px_ in range(2)], 0).contiguous()
    ops.conv2d([xg], wp4, sc, sh, out4, kh=2, kw=2, stride=1, pad=0, pad_yx=(1, 1), cout=Co, act=ops.ACT_RELU, Ho=H, Wo=W,
               out_scatter=(2, 2, 0, 0), nsub=4)
    assert torch.equal(out4, out)


@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (3, 2, 1)])
def test_maxpool(k, s, p):
    from centerpose_amd import ops
    x = torch.randn(2, 16, 13, 18)
    ref = F.max_pool2d(x, k, s, p)
    out = torch.empty(2, ref.shape[2], ref.shape[3], 16, device="cuda")
    ops.maxpool2d(_nhwc(x), out, k, s, p)
    assert torch.equal(out.permute(0, 3, 1, 2).cpu(), ref)


@pytest.mark.parametrize("f,B,C,H,W", [(2, 2, 32, 7, 9), (4, 2, 32, 7, 9), (2, 3, 64, 17, 5), (2, 2, 128, 8, 33)])
def test_dw_deconv_add(f, B, C, H, W):
    """IDAUp: up_i(proj(x)) + layers[i-1] (pose_dla_dcn.py:371-377); f = 2 and 4, strided (channel-padded) output views, with and
    without the addend."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(f + C + H)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, 2 * f, 2 * f, generator=g)
    add = torch.randn(B, C, H * f, W * f, generator=g)
    ref = F.conv_transpose2d(x, w, None, stride=f, padding=f // 2, groups=C) + add
    buf = torch.full((B, H * f, W * f, C + 16), float("nan"), device="cuda")
    out = buf[..., :C]
    ops.dw_deconv_add(_nhwc(x), ops.pack_dw_deconv_weight(w.cuda()), _nhwc(add), out, f)
    _close(out.permute(0, 3, 1, 2), ref, 1e-5)
    assert torch.isnan(buf[..., C:]).all()
    out2 = torch.empty(B, H * f, W * f, C, device="cuda")                     # no addend
    ops.dw_deconv_add(_nhwc(x), ops.pack_dw_deconv_weight(w.cuda()), None, out2, f)
    _close(out2.permute(0, 3, 1, 2), ref - add, 1e-5)


@pytest.mark.parametrize("B,C,H,W", [(1, 16, 5, 7), (3, 64, 9, 13), (2, 32, 16, 16)])
def test_dw_deconv2_kernel_equals_generic_kernel_bitwise(B, C, H, W, monkeypatch):
    """every f = 2 up-sampling runs on `dw_deconv2_add_kernel` (2 x 2 output patch per input pixel) and its "same taps in
    the same order, bit-identical" claim had no direct A/B.  CP_DWDECONV2=0 selects the generic kernel: both kernels, bit for bit, on
    odd H / W, B > 1, with / without the addend, and IN PLACE (add is out -- the engine may alias them, neither is __restrict__)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(B * 100 + C + H)
    x = _nhwc(torch.randn(B, C, H, W, generator=g))
    w = ops.pack_dw_deconv_weight(torch.randn(C, 1, 4, 4, generator=g).cuda())
    add = _nhwc(torch.randn(B, C, 2 * H, 2 * W, generator=g))
    got = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("CP_DWDECONV2", sw)
        o1 = torch.empty(B, 2 * H, 2 * W, C, device="cuda")
        la = ops.dw_deconv_add_launch(x, w, add, o1, 2)
        la.run()
        assert la.kernel == ("dw_deconv2_add_kernel" if sw == "1" else "dw_deconv_add_kernel")
        o2 = torch.empty_like(o1)
        ops.dw_deconv_add(x, w, None, o2, 2)
        o3 = add.clone()
        ops.dw_deconv_add(x, w, o3, o3, 2)                     # in place
        torch.cuda.synchronize()
        got[sw] = (o1, o2, o3)
    assert all(torch.equal(a, b) for a, b in zip(got["1"], got["0"]))
    assert torch.equal(got["1"][0], got["1"][2])                # in place == out of place


def test_sum_up():
    from centerpose_amd import ops
    a, b, c = torch.randn(2, 32, 16, 24), torch.randn(2, 32, 8, 12), torch.randn(2, 32, 4, 6)
    ref = F.relu(a + F.interpolate(b, scale_factor=2, mode="nearest") + F.interpolate(c, scale_factor=4, mode="nearest"))
    out = torch.empty(2, 16, 24, 32, device="cuda")
    ops.sum_up([_nhwc(a), _nhwc(b), _nhwc(c)], [0, 1, 2], out, True)
    _close(out.permute(0, 3, 1, 2), ref, 1e-6)


@pytest.mark.parametrize("nmem", [2, 3, 4])
def test_sum_up_group_equals_single_launches(nmem):
    """cp_sum_up_group_nhwc_f32 (round 6): the per-branch sums that end an HRNet module (pose_higher_hrnet.py:224-235, y_i = relu(sum_j
    fuse_ij(x_j))) as ONE launch -- members of different sizes, source counts and up-sampling factors, odd map sizes, channel-padded
    views -- BIT-IDENTICAL to one cp_sum_up_nhwc_f32 launch per member, and against torch."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(nmem)
    B = 2
    shapes = [(32, 24, 20), (64, 12, 10), (128, 6, 5), (256, 3, 3)][:nmem]          # (C, H, W) of the branches
    members, refs = [], []
    total = sum(B * H * W * C for C, H, W in shapes)
    whole = torch.full((total,), float("nan"), device="cuda")
    off = 0
    for i, (C, H, W) in enumerate(shapes):
        srcs, shifts, ref = [], [], 0
        for j in range(nmem):                       # a term per branch: same size (j <= i) or 2^(j - i) times smaller (j > i)
            sh = j - i if j > i else 0
            if (H >> sh) == 0 or (W >> sh) == 0 or H % (1 << sh) or W % (1 << sh):
                continue
            t = torch.randn(B, C, H >> sh, W >> sh, generator=g)
            ref = ref + (F.interpolate(t, scale_factor=1 << sh, mode="nearest") if sh else t)
            wide = torch.randn(B, H >> sh, W >> sh, C + 16, generator=g).cuda()     # a view with a larger pixel stride
            wide[..., :C] = _nhwc(t)
            srcs.append(wide[..., :C] if j % 2 else _nhwc(t))
            shifts.append(sh)
        out = whole[off:off + B * H * W * C].view(B, H, W, C)
        off += B * H * W * C
        members.append((srcs, shifts, out))
        refs.append(F.relu(ref))
    la = ops.sum_up_group_launch(members, whole, True)
    la.run()
    assert la.kernel == "sum_up_group_kernel" and not torch.isnan(whole).any()
    for (srcs, shifts, out), ref in zip(members, refs):
        _close(out.permute(0, 3, 1, 2), ref, 1e-6)
        single = torch.empty_like(out)
        ops.sum_up(srcs, shifts, single, True)
        assert torch.equal(single, out)


@pytest.mark.parametrize("C,k,stride,act", [(16, 3, 1, 0), (72, 5, 2, 1), (64, 3, 2, 3), (240, 5, 1, 3), (24, 3, 1, 4)])
def test_dwconv_bn_act(C, k, stride, act):
    """depthwise k x k + folded BN + {none, relu, h-swish, h-sigmoid} vs torch (mobilenetv3.py:119-121, shufflenetv2_dcn.py:67-88)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(C + k)
    B, H, W = 2, 13, 18
    x = torch.randn(B, C, H, W, generator=g) * 2
    w = torch.randn(C, 1, k, k, generator=g) * 0.3
    bn = _rand_bn(g, C)
    ref = _ref_bn(F.conv2d(x, w, None, stride, k // 2, 1, C), bn)
    ref = {0: ref, 1: F.relu(ref), 3: ref * F.relu6(ref + 3) / 6, 4: F.relu6(ref + 3) / 6}[act]
    Cp = (C + 15) // 16 * 16
    xp = torch.zeros(B, H, W, Cp)
    xp[..., :C] = x.permute(0, 2, 3, 1)
    gm, bt, mean, var = bn
    scale = gm / torch.sqrt(var + 1e-5)
    pad = lambda v: torch.cat([v, torch.zeros(Cp - C)]).cuda()
    wk = torch.cat([ops.pack_dw_weight(w), torch.zeros(k * k, Cp - C)], 1).contiguous().cuda()
    Ho, Wo = ref.shape[2:]
    out = torch.full((B, Ho, Wo, Cp), float("nan"), device="cuda")
    ops.dwconv2d(xp.cuda(), wk, pad(scale), pad(bt - mean * scale), out, k, stride, k // 2, act)
    _close(out[..., :C].permute(0, 3, 1, 2), ref, 1e-5)
    if act != 4:
        assert torch.equal(out[..., C:], torch.zeros_like(out[..., C:]))     # padding channels stay exact zeros


def test_squeeze_excite_pieces():
    """global average pool and x * se (+ shortcut) vs torch (SeModule, mobilenetv3.py:99-113,141-143)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 11, 7, 48, generator=g).cuda()
    sc = torch.randn(3, 11, 7, 48, generator=g).cuda()
    pooled = torch.empty(3, 1, 1, 48, device="cuda")
    ops.global_avgpool(x, pooled)
    _close(pooled, x.mean((1, 2), keepdim=True), 1e-6)
    se = torch.rand(3, 1, 1, 48, generator=g).cuda()
    out = torch.empty_like(x)
    ops.scale_add(x, se, sc, out)
    assert torch.equal(out, x * se + sc)
    ops.scale_add(x, se, None, out)
    assert torch.equal(out, x * se)


@pytest.mark.parametrize("h", [58, 116, 16, 29])
def test_channel_shuffle_concat(h):
    """channel_shuffle(cat(x1, x2), 2) (shufflenetv2_dcn.py:28-42) into the split layout; the halves come back as views."""
    from centerpose_amd import ops
    hp = (h + 15) // 16 * 16
    g = torch.Generator().manual_seed(h)
    x1, x2 = torch.randn(2, h, 5, 6, generator=g), torch.randn(2, h, 5, 6, generator=g)
    cat = torch.cat((x1, x2), 1)
    ref = cat.view(2, 2, h, 5, 6).transpose(1, 2).contiguous().view(2, 2 * h, 5, 6)
    a = torch.zeros(2, 5, 6, 2 * hp)
    a[..., :h] = x1.permute(0, 2, 3, 1)                   # x1 arrives as a half-view of a wider tensor (ld = 2 hp)
    b = torch.zeros(2, 5, 6, hp)
    b[..., :h] = x2.permute(0, 2, 3, 1)
    ad = a.cuda()
    out = torch.full((2, 5, 6, 2 * hp), float("nan"), device="cuda")
    ops.shuffle_concat(ad[..., :hp], b.cuda(), out, h, hp)
    o = out.cpu()
    assert torch.equal(o[..., :h].permute(0, 3, 1, 2), ref[:, :h]) and torch.equal(o[..., hp:hp + h].permute(0, 3, 1, 2), ref[:, h:])
    assert torch.equal(o[..., h:hp], torch.zeros(2, 5, 6, hp - h)) and torch.equal(o[..., hp + h:], torch.zeros(2, 5, 6, hp - h))


def test_dcn_v2_split_k_vs_scalar_oracle():
    """cp_dcn_desc.ksplit: split-K over the taps into raw partial sums + cp_splitk_reduce_f32 (fixed-order sum, bias, ReLU) ==
    the scalar oracle; S = 3 and the extreme S = 9 (one tap per block), ragged M, 64- and 128-wide N tiles; twice -> same bits."""
    from centerpose_amd import ops
    from oracle import dcn as odcn
    cases = [(64, 64, 9, 7, 3, 0), (32, 128, 6, 10, 9, 64128), (128, 256, 8, 8, 3, 64064), (48, 64, 5, 9, 2, 0)]
    for (C, Co, H, W, S, tile), sig in [(c, g) for c in cases for g in (False, True)]:
        x, w, b, off, m = _dcn_case(C + S, 2, C, Co, H, W, True)
        m_in = m
        if sig:              # the timed mode: mask logits in `om`, sigmoid inside the kernel
            m_in, m = _dcn_mask_logits(C + S, m.shape)
        ref = np.maximum(odcn.dcn_v2_forward_c(x, w, b, off, m), 0.0)
        om = torch.zeros(2, H, W, 32)
        om[..., :18] = torch.from_numpy(off).permute(0, 2, 3, 1)
        om[..., 18:27] = torch.from_numpy(m_in).permute(0, 2, 3, 1)
        wp = ops.pack_conv_weight(torch.from_numpy(w).cuda())
        ldw = wp.shape[0]
        sc, sh = ops.fold_bn(Co, None, torch.from_numpy(b).cuda())
        ws = torch.full((S, 2 * H * W, ldw), float("nan"), device="cuda")
        out = torch.full((2, H, W, Co + 4), float("nan"), device="cuda")
        xs, oms = _nhwc(torch.from_numpy(x)), om.cuda()
        la = ops.dcn_v2_launch(xs, oms, wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw,
                               om_sigmoid=sig, tile=tile, ksplit=S)
        lb = ops.splitk_reduce_launch(ws, sc, sh, out[..., :Co], cout=Co, act=ops.ACT_RELU)
        la.run(); lb.run()
        first = out.clone()
        la.run(); lb.run()
        assert torch.equal(first[..., :Co], out[..., :Co]) and torch.isnan(out[..., Co:]).all()
        _close(out[..., :Co].permute(0, 3, 1, 2), torch.from_numpy(ref), 1e-4)


@pytest.mark.parametrize("C,Co,H,W,big,tile", [(16, 64, 12, 10, True, 0), (64, 64, 16, 16, False, 128064),
                                               (32, 32, 9, 13, True, 128032), (128, 128, 8, 8, False, 64064),
                                               (64, 64, 11, 13, True, 64064), (32, 128, 9, 16, False, 64128),
                                               # even / odd k-step counts, ragged M, 64x128 tile, non-multiple-of-32 channels
                                               (16, 64, 9, 7, True, 64064), (48, 128, 6, 10, True, 64128),
                                               (128, 256, 8, 8, False, 64128), (32, 64, 12, 12, True, 128064),
                                               (96, 128, 6, 10, True, 64032), (48, 64, 5, 9, True, 64032),
                                               (128, 64, 11, 13, True, 0), (256, 64, 5, 6, True, 0)])
@pytest.mark.parametrize("sig", [False, True], ids=["mask", "logits"])
def test_dcn_v2_vs_scalar_oracle(C, Co, H, W, big, tile, sig):
    """sig=True is the mode of every in-plan launch (the timed path): `om` carries mask LOGITS and the kernel applies the sigmoid
    (v_rcp_f32(1 + exp(-x))); reference = torch.sigmoid in float32 -> the scalar oracle, at the same 1e-4 (SURVEY 8d gate 2)."""
    from centerpose_amd import ops
    from oracle import dcn as odcn
    x, w, b, off, m = _dcn_case(C + H, 2, C, Co, H, W, big)
    m_in = m
    if sig:
        m_in, m = _dcn_mask_logits(C + H, m.shape)
    ref = odcn.dcn_v2_forward_c(x, w, b, off, m)
    om = torch.zeros(2, H, W, 32)
    om[..., :18] = torch.from_numpy(off).permute(0, 2, 3, 1)
    om[..., 18:27] = torch.from_numpy(m_in).permute(0, 2, 3, 1)
    sc, sh = ops.fold_bn(Co, None, torch.from_numpy(b).cuda())
    out = torch.empty(2, H, W, Co, device="cuda")
    ops.dcn_v2(_nhwc(torch.from_numpy(x)), om.cuda(), ops.pack_conv_weight(torch.from_numpy(w).cuda()), sc, sh, out,
               cout=Co, om_sigmoid=sig, tile=tile)
    _close(out.permute(0, 3, 1, 2), torch.from_numpy(ref), 1e-4)


def test_dcn_zero_offset_identity():
    """The reference's only known-answer check (DCNv2/test.py:31-66): zero offsets, mask 0.5 =>
    2 * DCN(x) == conv(x)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 16, 10, 10, generator=g)
    w = torch.randn(32, 16, 3, 3, generator=g) * 0.1
    om = torch.zeros(2, 10, 10, 32)
    om[..., 18:27] = 0.5
    sc, sh = ops.fold_bn(32, None, torch.zeros(32).cuda())
    out = torch.empty(2, 10, 10, 32, device="cuda")
    ops.dcn_v2(_nhwc(x), om.cuda(), ops.pack_conv_weight(w.cuda()), sc, sh, out, cout=32, om_sigmoid=False)
    _close(2 * out.permute(0, 3, 1, 2), F.conv2d(x, w, None, 1, 1), 1e-5)


@pytest.mark.parametrize("C,Co,k,s,p,d", [(8, 6, 3, 1, 1, 1), (16, 32, 3, 2, 1, 1), (32, 16, 3, 1, 2, 2), (5, 7, 1, 1, 0, 1)])
def test_dcn_v2_forward_ext_dropin(C, Co, k, s, p, d):
    """reference FFI signature (DCNv2/src/dcn_v2.h:9-23): NCHW in, new NCHW tensor out, any stride/pad/dilation."""
    from centerpose_amd import dcn_v2_ext
    from oracle import dcn as odcn
    r = np.random.RandomState(C * 7 + k)
    B, H, W = 2, 11, 9
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, k, k) * 0.2).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * k * k, Ho, Wo) * 2).astype(np.float32)
    m = r.rand(B, k * k, Ho, Wo).astype(np.float32)
    ref = odcn.dcn_v2_forward_c(x, w, b, off, m, k, k, s, s, p, p, d, d, 1)
    t = [torch.from_numpy(a).cuda() for a in (x, w, b, off, m)]
    out = dcn_v2_ext.dcn_v2_forward(*t, k, k, s, s, p, p, d, d, 1)
    assert out.shape == ref.shape and out.is_cuda
    _close(out, torch.from_numpy(ref), 1e-4)
    with pytest.raises(RuntimeError):
        dcn_v2_ext.dcn_v2_forward(t[0].cpu(), *t[1:], k, k, s, s, p, p, d, d, 1)


@pytest.mark.parametrize("C,Co,k,s,p,d", [(8, 6, 3, 1, 1, 1), (16, 32, 3, 2, 1, 1), (64, 64, 3, 1, 1, 1), (5, 7, 1, 1, 0, 1)])
def test_pybind_ext_dcn_v2_forward(C, Co, k, s, p, d):
    """The compiled pybind module `_ext` (torch cpp_extension; DCNv2/src/vision.cpp:4-9) with the reference's 14-argument call."""
    from centerpose_amd import _ext
    from oracle import dcn as odcn
    r = np.random.RandomState(C * 5 + k)
    B, H, W = 2, 11, 9
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, k, k) * 0.2).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * k * k, Ho, Wo) * 2).astype(np.float32)
    m = r.rand(B, k * k, Ho, Wo).astype(np.float32)
    ref = odcn.dcn_v2_forward_c(x, w, b, off, m, k, k, s, s, p, p, d, d, 1)
    t = [torch.from_numpy(a).cuda() for a in (x, w, b, off, m)]
    out = _ext.dcn_v2_forward(*t, k, k, s, s, p, p, d, d, 1)
    assert out.shape == ref.shape and out.is_cuda
    _close(out, torch.from_numpy(ref), 1e-4)
    with pytest.raises(RuntimeError):
        _ext.dcn_v2_backward(*t, t[0], k, k, s, s, p, p, d, d, 1)


@pytest.mark.parametrize("C,Co,dg,k,s,p,d", [(32, 64, 2, 3, 1, 1, 1), (64, 64, 4, 3, 1, 1, 1), (96, 128, 2, 3, 2, 1, 1), (12, 7, 3, 3, 1, 2, 2),
                                             (20, 40, 2, 1, 1, 0, 1), (64, 32, 1, 3, 1, 1, 1)])
@pytest.mark.parametrize("face", ["python", "pybind"])
def test_dcn_v2_forward_deformable_groups(C, Co, dg, k, s, p, d, face):
    """deformable_group > 1 through both faces of the reference FFI (the one argument of the 14 that used to raise).
    Reference semantics dcn_v2_im2col_cuda.cu:153,162-164: channel c samples with group c // (C // dg); offset channels
    [g*2*kk, (g+1)*2*kk), mask channels [g*kk, (g+1)*kk).  Oracle: oracle/dcn_ref.c (implements dg).  Channel counts per group that
    are not multiples of 16 (12 / 3 = 4, 20 / 2 = 10) exercise the per-group padding of the wrappers."""
    from oracle import dcn as odcn
    if face == "python":
        from centerpose_amd import dcn_v2_ext as ext
    else:
        from centerpose_amd import _ext as ext
    r = np.random.RandomState(C * 3 + dg)
    B, H, W = 2, 10, 13
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, k, k) * 0.2).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * dg * k * k, Ho, Wo) * 2.5).astype(np.float32)
    off[0, :, 0, 0] = 3 * H                     # far out of range in every group
    off[-1, 0::2, 1, 1] = -1.0                  # on the boundary rule
    m = r.rand(B, dg * k * k, Ho, Wo).astype(np.float32)
    ref = odcn.dcn_v2_forward_c(x, w, b, off, m, k, k, s, s, p, p, d, d, dg)
    if dg > 1:                                  # the groups really differ: group 0's offsets for everyone is another answer
        off1 = np.tile(off[:, :2 * k * k], (1, dg, 1, 1))
        assert np.abs(odcn.dcn_v2_forward_c(x, w, b, off1, m, k, k, s, s, p, p, d, d, dg) - ref).max() > 1e-2
    t = [torch.from_numpy(a).cuda() for a in (x, w, b, off, m)]
    out = ext.dcn_v2_forward(*t, k, k, s, s, p, p, d, d, dg)
    assert out.shape == ref.shape and out.is_cuda
    _close(out, torch.from_numpy(ref), 1e-4)
    with pytest.raises(RuntimeError):
        ext.dcn_v2_forward(*t, k, k, s, s, p, p, d, d, dg + 7 if C % (dg + 7) else C + 1)      # C not divisible by the group count


@pytest.mark.parametrize("C,Co,kh,kw,sh,sw,ph,pw,dh,dw,dg", [
    (16, 24, 3, 3, 2, 1, 1, 2, 1, 2, 1),        # every pair different: stride (2, 1), pad (1, 2), dilation (1, 2)
    (32, 16, 1, 3, 1, 2, 0, 1, 1, 1, 2),        # 1 x 3 kernel, two deformable groups
    (8, 12, 5, 5, 1, 1, 2, 2, 1, 1, 1),         # 25 taps (rounds 1-5 stopped at 9)
    (16, 8, 3, 5, 2, 2, 3, 1, 2, 1, 1),         # 15 taps, stride 2, pad (3, 1), dilation (2, 1)
    (16, 16, 7, 7, 1, 1, 3, 3, 1, 1, 1),        # 49 taps
])
@pytest.mark.parametrize("face", ["python", "pybind"])
def test_dcn_v2_forward_full_argument_space(C, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, face):
    """the reference's `dcn_v2_forward` takes INDEPENDENT stride_h / stride_w, pad_h / pad_w, dilation_h / dilation_w
    and any kernel size (DCNv2/src/cuda/dcn_v2_cuda.cu:43-57,77-87; im2col :125-195 walks kernel_h x kernel_w taps).  Rounds 1-5's
    wrappers refused non-square parameters and more than 9 taps although the kernel carries every parameter per axis; the tap
    capacity of the sampling-record rows is a run-time value now.  Both FFI faces against oracle/dcn_ref.c, offsets incl. far
    out-of-range and boundary probes."""
    from oracle import dcn as odcn
    if face == "python":
        from centerpose_amd import dcn_v2_ext as ext
    else:
        from centerpose_amd import _ext as ext
    r = np.random.RandomState(C + 3 * kh + 5 * kw + sh)
    B, H, W = 2, 12, 15
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    kk = kh * kw
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, kh, kw) * 0.2).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * dg * kk, Ho, Wo) * 2.0).astype(np.float32)
    off[0, :, 0, 0] = 4 * H
    off[-1, 0::2, -1, -1] = -1.0
    m = r.rand(B, dg * kk, Ho, Wo).astype(np.float32)
    ref = odcn.dcn_v2_forward_c(x, w, b, off, m, kh, kw, sh, sw, ph, pw, dh, dw, dg)
    # the axes are really independent: the transposed parameter pairs give another answer (or another shape)
    if (sh, ph, dh) != (sw, pw, dw) and kh == kw:
        alt_shape = ((H + 2 * pw - (dw * (kh - 1) + 1)) // sw + 1, (W + 2 * ph - (dh * (kw - 1) + 1)) // sh + 1)
        assert alt_shape != (Ho, Wo) or np.abs(odcn.dcn_v2_forward_c(x, w, b, off, m, kh, kw, sw, sh, pw, ph, dw, dh, dg) - ref).max() > 1e-2
    t = [torch.from_numpy(a).cuda() for a in (x, w, b, off, m)]
    out = ext.dcn_v2_forward(*t, kh, kw, sh, sw, ph, pw, dh, dw, dg)
    assert tuple(out.shape) == (B, Co, Ho, Wo) == ref.shape and out.is_cuda
    _close(out, torch.from_numpy(ref), 1e-4)
    with pytest.raises(RuntimeError):
        ext.dcn_v2_forward(*t, kh, kw, 0, sw, ph, pw, dh, dw, dg)                     # stride 0
    with pytest.raises(RuntimeError):
        ext.dcn_v2_forward(*t, kh + 1, kw, sh, sw, ph, pw, dh, dw, dg)                # kernel size does not match the weight


def test_dcn_v2_forward_random_argument_fuzz():
    """Seeded fuzz over the argument space of `dcn_v2_forward` (DCNv2/src/cuda/dcn_v2_cuda.cu:43-57): 24 random combinations of channel
    counts, kernel size (1..5 per axis), stride (1..3), pad (0..3), dilation (1..2) per axis and deformable groups, through the pybind
    face against oracle/dcn_ref.c -- every output shape and every value (1e-4)."""
    from centerpose_amd import _ext
    from oracle import dcn as odcn
    r = np.random.RandomState(2024)
    done = 0
    while done < 24:
        dg = int(r.choice([1, 1, 2, 3]))
        C = dg * int(r.choice([4, 8, 16, 24]))
        Co = int(r.choice([3, 8, 17, 40]))
        kh, kw = int(r.randint(1, 6)), int(r.randint(1, 6))
        sh, sw = int(r.randint(1, 4)), int(r.randint(1, 4))
        ph, pw = int(r.randint(0, 4)), int(r.randint(0, 4))
        dh, dw = int(r.randint(1, 3)), int(r.randint(1, 3))
        B, H, W = 2, int(r.randint(7, 15)), int(r.randint(7, 15))
        Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
        Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
        if Ho < 1 or Wo < 1:
            continue
        kk = kh * kw
        x = r.randn(B, C, H, W).astype(np.float32)
        w = (r.randn(Co, C, kh, kw) / np.sqrt(C * kk)).astype(np.float32)
        b = r.randn(Co).astype(np.float32)
        off = (r.randn(B, 2 * dg * kk, Ho, Wo) * 1.5).astype(np.float32)
        m = r.rand(B, dg * kk, Ho, Wo).astype(np.float32)
        ref = odcn.dcn_v2_forward_c(x, w, b, off, m, kh, kw, sh, sw, ph, pw, dh, dw, dg)
        out = _ext.dcn_v2_forward(*(torch.from_numpy(a).cuda() for a in (x, w, b, off, m)), kh, kw, sh, sw, ph, pw, dh, dw, dg)
        assert tuple(out.shape) == ref.shape, (C, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg)
        err = (out.cpu() - torch.from_numpy(ref)).abs().max().item()
        assert err <= 1e-4 * max(1.0, float(np.abs(ref).max())), ((C, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg), err)
        done += 1


@pytest.mark.parametrize("face", ["python", "pybind"])
def test_dcn_v2_forward_follows_every_kind_of_parameter_update(face):
    """The ext faces pack the weights with one device launch per call (round 5; rounds 3-4 cached the pack on (data_ptr, _version)).
    ADVICE r4: an edit through `.data` -- what EMA / legacy loaders and the reference's own reset_parameters do (DCNv2/dcn_v2.py:44-52)
    -- does not bump the version counter and was invisible to that cache; `_version` raises on inference tensors; a pack built on one
    stream was read by others without an event.  All of these must simply work now, next to versioned in-place updates."""
    from oracle import dcn as odcn
    if face == "python":
        from centerpose_amd import dcn_v2_ext as ext
    else:
        from centerpose_amd import _ext as ext
    r = np.random.RandomState(3)
    x, off, m = r.randn(1, 32, 8, 8).astype(np.float32), r.randn(1, 18, 8, 8).astype(np.float32), r.rand(1, 9, 8, 8).astype(np.float32)
    w = torch.nn.Parameter(torch.from_numpy((r.randn(32, 32, 3, 3) * 0.2).astype(np.float32)).cuda())
    b = torch.nn.Parameter(torch.from_numpy(r.randn(32).astype(np.float32)).cuda())
    t = [torch.from_numpy(a).cuda() for a in (x, off, m)]
    call = lambda: ext.dcn_v2_forward(t[0], w, b, t[1], t[2], 3, 3, 1, 1, 1, 1, 1, 1, 1)
    want = lambda: torch.from_numpy(odcn.dcn_v2_forward_c(x, w.detach().cpu().numpy(), b.detach().cpu().numpy(), off, m))
    o1, o2 = call(), call()
    assert torch.equal(o1, o2) and not o1.requires_grad
    _close(o1, want(), 1e-4)
    with torch.no_grad():                       # versioned in-place update (optimizer step, load_state_dict)
        w.mul_(0.5)
        b.add_(1.0)
    o3 = call()
    _close(o3, want(), 1e-4)
    assert not torch.equal(o3, o1)
    v = w._version                              # `.data` edits: the version counter does NOT move
    w.data.mul_(-2.0)
    b.data.copy_(torch.from_numpy(r.randn(32).astype(np.float32)))
    assert w._version == v
    o4 = call()
    _close(o4, want(), 1e-4)
    assert not torch.equal(o4, o3)
    with torch.inference_mode():                # inference tensors have no version counter at all
        wi, bi = (w.detach() * 1.5).contiguous(), b.detach() + 0.25
        oi = ext.dcn_v2_forward(t[0], wi, bi, t[1], t[2], 3, 3, 1, 1, 1, 1, 1, 1, 1)
        ref = odcn.dcn_v2_forward_c(x, wi.cpu().numpy(), bi.cpu().numpy(), off, m)
    _close(oi, torch.from_numpy(ref), 1e-4)
    side = torch.cuda.Stream()                  # another stream: the pack is enqueued on the caller's stream, nothing is shared
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o5 = call()
    side.synchronize()
    assert torch.equal(o5, o4)


@pytest.mark.parametrize("face", ["python", "pybind"])
def test_ext_exports_the_reference_modules_four_names(face):
    """DCNv2/src/vision.cpp:6-9: dcn_v2_forward, dcn_v2_backward, dcn_v2_psroi_pooling_forward / _backward.  The last three raise
    a clear RuntimeError (inference only / not on the hot path) instead of failing the attribute lookup."""
    if face == "python":
        from centerpose_amd import dcn_v2_ext as ext
    else:
        from centerpose_amd import _ext as ext
    assert callable(ext.dcn_v2_forward)
    for name in ("dcn_v2_backward", "dcn_v2_psroi_pooling_forward", "dcn_v2_psroi_pooling_backward"):
        with pytest.raises(RuntimeError, match="hot path"):
            getattr(ext, name)(*([None] * 15))


@pytest.mark.parametrize("C,Co,dg,tile,S", [(64, 64, 2, 0, 1), (128, 128, 4, 64128, 1), (64, 64, 2, 0, 3), (96, 64, 3, 128064, 1)])
def test_dcn_v2_kernel_deformable_groups_vs_scalar_oracle(C, Co, dg, tile, S):
    """cp_dcn_desc.dg at the kernel level (NHWC `om` with per-group offsets then per-group mask LOGITS, om_sigmoid=True), incl. the
    split-K form and the 64x128 / 128x64 tiles, against the scalar oracle."""
    from centerpose_amd import ops
    from oracle import dcn as odcn
    r = np.random.RandomState(C + dg + S)
    B, H, W, kk = 2, 9, 12, 9
    x = r.randn(B, C, H, W).astype(np.float32)
    w = (r.randn(Co, C, 3, 3) / (3 * C ** 0.5)).astype(np.float32)
    b = r.randn(Co).astype(np.float32)
    off = (r.randn(B, 2 * dg * kk, H, W) * 3.0).astype(np.float32)
    lg, m = _dcn_mask_logits(C + dg, (B, dg * kk, H, W))
    ref = np.maximum(odcn.dcn_v2_forward_c(x, w, b, off, m, 3, 3, 1, 1, 1, 1, 1, 1, dg), 0.0)
    omld = ops.round_up(3 * dg * kk, 4)
    om = torch.zeros(B, H, W, omld)
    om[..., :2 * dg * kk] = torch.from_numpy(off).permute(0, 2, 3, 1)
    om[..., 2 * dg * kk:3 * dg * kk] = torch.from_numpy(lg).permute(0, 2, 3, 1)
    wp = ops.pack_conv_weight(torch.from_numpy(w).cuda())
    sc, sh = ops.fold_bn(Co, None, torch.from_numpy(b).cuda())
    out = torch.empty(B, H, W, Co, device="cuda")
    if S > 1:
        ldw = wp.shape[0]
        ws = torch.full((S, B * H * W, ldw), float("nan"), device="cuda")
        ops.dcn_v2_launch(_nhwc(torch.from_numpy(x)), om.cuda(), wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws,
                          cout=ldw, om_sigmoid=True, tile=tile, ksplit=S, dg=dg).run()
        ops.splitk_reduce_launch(ws, sc, sh, out, cout=Co, act=ops.ACT_RELU).run()
    else:
        ops.dcn_v2(_nhwc(torch.from_numpy(x)), om.cuda(), wp, sc, sh, out, cout=Co, om_sigmoid=True, act=ops.ACT_RELU, tile=tile, dg=dg)
    _close(out.permute(0, 3, 1, 2), torch.from_numpy(ref), 1e-4)


# --- the HIP kernel against the REFERENCE's own im2col text ------------------------------------------------------------------------
# tests/golden/dcn_ref_<name>.npz: float32 outputs of oracle.dcn.dcn_v2_forward_ref (the reference's dmcn_im2col_bilinear /
# modulated_deformable_im2col_gpu_kernel compiled for the CPU, GEMM in float64), made by tests/golden/make_golden_dcn.py; inputs from
# tests/cases.py.  Same gate as the oracle tests above: 1e-4 * max|ref| (SURVEY 8d gate 2).  Worst errors: profiles/dcn_reference_pin.txt.

_DCN_FIXTURES = cases.dcn_fixtures()


def _dcn_golden(name, golden_dir):
    import os
    path = os.path.join(golden_dir, "dcn_ref_%s.npz" % name)
    assert os.path.exists(path), "missing reference fixture " + path
    with np.load(path) as z:
        return z["out"]


def _close_report(what, out, ref, tol=1e-4):
    out, ref = out.detach().cpu().double(), torch.from_numpy(np.ascontiguousarray(ref)).double()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err, scale = (out - ref).abs().max().item(), max(ref.abs().max().item(), 1e-6)
    print("\n%s: max err %.3e = %.3e of max|ref| %.3e (gate %.0e)" % (what, err, err / scale, scale, tol))
    assert err <= tol * scale, "%s: max err %.3e (scale %.3e)" % (what, err, scale)


def _dcn_kernel_run(c, tile, S=1, act=0):
    """One cp_dcn launch (S == 1) or split-K launch + cp_splitk_reduce_f32 (S > 1) on a tests/cases.py DCN case -> NCHW view."""
    from centerpose_amd import ops
    x, w, b, off = c["x"], c["w"], c["b"], c["off"]
    dg = c["args"][8]
    sig = c["logits"] is not None
    m_in = c["logits"] if sig else c["m"]
    B, C, H, W = x.shape
    Co, kk = w.shape[0], 9
    om = torch.zeros(B, H, W, ops.round_up(3 * dg * kk, 4) if dg > 1 else 32)
    om[..., :2 * dg * kk] = torch.from_numpy(off).permute(0, 2, 3, 1)
    om[..., 2 * dg * kk:3 * dg * kk] = torch.from_numpy(m_in).permute(0, 2, 3, 1)
    wp = ops.pack_conv_weight(torch.from_numpy(w).cuda())
    sc, sh = ops.fold_bn(Co, None, torch.from_numpy(b).cuda())
    out = torch.full((B, H, W, Co), float("nan"), device="cuda")
    xs = _nhwc(torch.from_numpy(x))
    if S > 1:
        ldw = wp.shape[0]
        ws = torch.full((S, B * H * W, ldw), float("nan"), device="cuda")
        ops.dcn_v2_launch(xs, om.cuda(), wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw,
                          om_sigmoid=sig, tile=tile, ksplit=S, dg=dg).run()
        ops.splitk_reduce_launch(ws, sc, sh, out, cout=Co, act=act).run()
    else:
        ops.dcn_v2(xs, om.cuda(), wp, sc, sh, out, cout=Co, om_sigmoid=sig, act=act, tile=tile, dg=dg)
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize("C,Co,H,W,big,tile,mode",
                         [r + ("mask",) for r in cases.DCN_KERNEL_SHAPES] + [r + ("logits",) for r in cases.DCN_FIXTURE_LOGITS_SHAPES])
def test_dcn_v2_vs_reference_golden(C, Co, H, W, big, tile, mode, golden_dir):
    """Every shape of test_dcn_v2_vs_scalar_oracle in mask mode and one shape per tile code (0, 64064, 64128, 128064, 128032, 64032)
    in logits mode (torch.sigmoid in float32 before the reference call, DCNv2/dcn_v2.py:117-127; the kernel applies its own)."""
    name = "kernel_%d_%d_%dx%d_%s" % (C, Co, H, W, mode)
    c = _DCN_FIXTURES[name]()
    assert (c["logits"] is not None) == (mode == "logits")
    _close_report(name, _dcn_kernel_run(c, tile), _dcn_golden(name, golden_dir))


@pytest.mark.parametrize("C,Co,H,W,S,tile", cases.DCN_SPLITK_SHAPES)
def test_dcn_v2_split_k_vs_reference_golden(C, Co, H, W, S, tile, golden_dir):
    """Split-K over the taps + cp_splitk_reduce_f32 (bias, ReLU) against max(reference, 0)."""
    from centerpose_amd import ops
    name = "splitk_%d_%d_%dx%d_s%d" % (C, Co, H, W, S)
    _close_report(name, _dcn_kernel_run(_DCN_FIXTURES[name](), tile, S, ops.ACT_RELU), np.maximum(_dcn_golden(name, golden_dir), 0.0))


@pytest.mark.parametrize("C,Co,dg,tile,S", cases.DCN_KERNEL_DG_SHAPES)
def test_dcn_v2_kernel_deformable_groups_vs_reference_golden(C, Co, dg, tile, S, golden_dir):
    """cp_dcn_desc.dg > 1 (mask logits, ReLU; one row through split-K) against max(reference, 0)."""
    from centerpose_amd import ops
    name = "kerneldg_%d_%d_g%d_s%d" % (C, Co, dg, S)
    _close_report(name, _dcn_kernel_run(_DCN_FIXTURES[name](), tile, S, ops.ACT_RELU), np.maximum(_dcn_golden(name, golden_dir), 0.0))


@pytest.mark.parametrize("name", [n for n in sorted(_DCN_FIXTURES) if n.startswith(("fullargs_", "lattice_"))])
@pytest.mark.parametrize("face", ["python", "pybind"])
def test_dcn_v2_forward_vs_reference_golden(name, face, golden_dir):
    """The full-argument-space rows and the boundary lattice (coordinates exactly on -1, just above it, 0, H-1, just below H, H, far
    out: tests/cases.py::dcn_lattice_case) through both faces of the reference FFI."""
    if face == "python":
        from centerpose_amd import dcn_v2_ext as ext
    else:
        from centerpose_amd import _ext as ext
    c = _DCN_FIXTURES[name]()
    out = ext.dcn_v2_forward(*(torch.from_numpy(c[k]).cuda() for k in ("x", "w", "b", "off", "m")), *c["args"])
    assert out.is_cuda
    _close_report("%s[%s]" % (name, face), out, _dcn_golden(name, golden_dir))


def test_dcn_reference_golden_all_used(golden_dir):
    """No fixture is left out: the four tests above name every committed dcn_ref_*.npz."""
    import os
    used = {"kernel_%d_%d_%dx%d_mask" % r[:4] for r in cases.DCN_KERNEL_SHAPES} | {"kernel_%d_%d_%dx%d_logits" % r[:4] for r in cases.DCN_FIXTURE_LOGITS_SHAPES}
    used |= {"splitk_%d_%d_%dx%d_s%d" % r[:5] for r in cases.DCN_SPLITK_SHAPES} | {"kerneldg_%d_%d_g%d_s%d" % (r[0], r[1], r[2], r[4]) for r in cases.DCN_KERNEL_DG_SHAPES}
    used |= {n for n in _DCN_FIXTURES if n.startswith(("fullargs_", "lattice_"))}
    have = {f[len("dcn_ref_"):-len(".npz")] for f in os.listdir(golden_dir) if f.startswith("dcn_ref_") and f.endswith(".npz")}
    assert used == have == set(_DCN_FIXTURES)


@pytest.mark.parametrize("cin,cout,hw,B", [(16, 16, (24, 40), 2), (16, 64, (8, 16), 1), (64, 64, (20, 28), 3), (32, 27, (16, 16), 2),
                                           (48, 128, (9, 35), 2), (128, 192, (16, 16), 2)])
def test_conv3x3_patch_kernel(cin, cout, hw, B):
    """LDS-resident halo-patch kernel (tile=3) for 3x3/s1/p1: edges, ragged tiles, residual, all N tiles;
    must agree with the generic implicit-GEMM kernel and the torch-CPU reference."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    H, W = hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bn = _rand_bn(g, cout)
    res = torch.randn(B, cout, H, W, generator=g)
    ref = F.relu(_ref_bn(F.conv2d(x, w, None, 1, 1), bn) + res)
    wp = ops.pack_conv_weight(w.cuda())
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    cst = wp.shape[0] if cout == 27 else cout
    out = torch.full((B, H, W, cst), float("nan"), device="cuda")
    resn = torch.zeros(B, H, W, cst)
    resn[..., :cout] = res.permute(0, 2, 3, 1)
    ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=3, kw=3, stride=1, pad=1, cout=cst, act=ops.ACT_RELU, res=resn.cuda(), tile=3)
    _close(out[..., :cout].permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("cout,s,hw,B,act,with_res,view", [
    (16, 1, (40, 72), 2, 1, False, False), (32, 2, (37, 70), 2, 1, False, False), (16, 1, (16, 32), 1, 0, True, False),
    (32, 2, (16, 32), 3, 1, True, True), (32, 1, (19, 45), 2, 1, True, False), (16, 2, (33, 17), 2, 0, False, True),
    (16, 1, (5, 3), 1, 1, False, False), (32, 2, (2, 3), 1, 1, False, False), (32, 2, (64, 64), 2, 1, False, False)])
def test_conv3x3_c16_kernel(cout, s, hw, B, act, with_res, view):
    """Weights-in-registers kernel for 16-channel 3x3 convs (tile=16; DLA level0 / level1, pose_dla_dcn.py:234-246): stride 1 / 2,
    16 / 32 outputs, image edges and ragged tiles, residual, output written into a channel view of a wider tensor; against the
    torch-CPU reference and bit-compared with nothing else (its summation order is its own)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cout * 7 + s + hw[0])
    H, W = hw
    x = torch.randn(B, 16, H, W, generator=g)
    w = torch.randn(cout, 16, 3, 3, generator=g) / 12.0
    bn = _rand_bn(g, cout)
    ref = _ref_bn(F.conv2d(x, w, None, s, 1), bn)
    Ho, Wo = ref.shape[2:]
    res = torch.randn(B, cout, Ho, Wo, generator=g) if with_res else None
    if with_res:
        ref = ref + res
    if act:
        ref = F.relu(ref)
    wp = ops.pack_conv_weight(w.cuda())
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    full = torch.full((B, Ho, Wo, cout + (16 if view else 0)), float("nan"), device="cuda")
    out = full[..., 16:] if view else full
    ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=3, kw=3, stride=s, pad=1, cout=cout, act=ops.ACT_RELU if act else ops.ACT_NONE,
               res=_nhwc(res) if with_res else None, tile=16)
    from centerpose_amd import _lib
    assert _lib.lib().cp_last_kernel().decode().startswith("conv3x3_c16_kernel")
    _close(out.permute(0, 3, 1, 2), ref)
    if view:
        assert torch.isnan(full[..., :16]).all()
    # tile = 0 (auto) must pick the same kernel for this shape: same bits
    out2 = torch.empty(B, Ho, Wo, cout, device="cuda")
    ops.conv2d([_nhwc(x)], wp, sc, sh, out2, kh=3, kw=3, stride=s, pad=1, cout=cout, act=ops.ACT_RELU if act else ops.ACT_NONE,
               res=_nhwc(res) if with_res else None)
    assert torch.equal(out2, out.contiguous())


@pytest.mark.parametrize("cin,cout,hw,B,nt", [(16, 32, (24, 40), 2, 0), (64, 64, (20, 28), 3, 11), (64, 64, (20, 28), 3, 12),
                                              (64, 64, (20, 28), 3, 21), (32, 27, (16, 16), 2, 0), (32, 27, (19, 16), 2, 11),
                                              (48, 128, (9, 35), 2, 12), (48, 128, (9, 35), 2, 21), (128, 192, (16, 16), 2, 0),
                                              (64, 256, (32, 32), 1, 21), (256, 96, (8, 8), 2, 11),
                                              (64, 256, (20, 28), 2, 6401), (64, 256, (9, 35), 1, 6403), (64, 64, (16, 16), 2, 6402),
                                              (64, 27, (19, 16), 2, 6400), (64, 96, (8, 8), 2, 6408)])
def test_conv3x3_winograd_kernel(cin, cout, hw, B, nt):
    """fused Winograd F(2x2,3x3) kernel: odd sizes, ragged tiles, residual, ragged channel tiles, scalar-store tail;
    against the torch-CPU fp32 direct convolution.  Tolerance 2e-4 * max|ref| like the direct kernels (measured
    error is ~3e-6 relative: fp32 transforms, fp32 MFMA accumulate)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(7 * cin + cout)
    H, W = hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bn = _rand_bn(g, cout)
    res = torch.randn(B, cout, H, W, generator=g) if cout != 96 else None
    y = _ref_bn(F.conv2d(x, w, None, 1, 1), bn)
    ref = F.relu(y + res) if res is not None else y
    wp = ops.pack_conv_weight(w.cuda())
    u = ops.pack_wino_weight(wp, cin, cout)
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    ld = 32 if cout == 27 else cout
    buf = torch.full((B, H, W, ld), float("nan"), device="cuda")
    out = buf[..., :cout]
    resn = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    ops.conv2d([_nhwc(x)], wp, sc, sh, out, kh=3, kw=3, stride=1, pad=1, cout=cout,
               act=ops.ACT_RELU if res is not None else ops.ACT_NONE, res=resn, tile=nt, wino=u)
    _close(out.permute(0, 3, 1, 2), ref)
    if ld != cout:
        assert torch.isnan(buf[..., cout:]).all()      # nothing stored past Cout


@pytest.mark.parametrize("B,H,W,hc,n2,act2", [(2, 32, 48, 256, 1, 2), (1, 37, 45, 256, 2, 0), (3, 8, 16, 128, 2, 0), (1, 19, 9, 64 * 5, 1, 2),
                                               # second MFMA phase (round 3): hm_hp 17 (+ sigmoid), hps 34 = 32 MFMA + 2 register path,
                                               # 33, a full 32, 3 (smallest MM case), ragged tiles, one channel tile only
                                               (2, 32, 48, 256, 17, 2), (1, 37, 45, 256, 34, 0), (3, 8, 16, 128, 33, 0), (1, 19, 9, 64 * 5, 32, 0),
                                               (2, 16, 16, 256, 3, 2), (1, 9, 21, 32, 34, 0), (16, 128, 128, 256, 34, 0)])
@pytest.mark.parametrize("w24", [False, True], ids=["f2x2", "f2x4"])
def test_head3x3_1x1_fused(B, H, W, hc, n2, act2, w24):
    """(w24: the same launch on the F(2x4,3x3) head kernel -- head_wino24.hip, eight waves per 16x16-pixel block, round 4.)
    One KeypointHead branch in ONE launch (keypoint.py:14-37: conv3x3 + bias -> ReLU -> conv1x1 + bias; hm / hm_hp get their
    sigmoid, multi_pose.py:35-37): <= 2 outputs ride in the Winograd kernel's epilogue registers, 3..34 outputs (hm_hp, hps) go
    through a second MFMA phase over the LDS-resident ReLU'd tile.  Ragged tiles; the last case is the bench's own shape."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(B * 100 + H + n2)
    x = torch.randn(B, 64, H, W, generator=g)
    w3 = torch.randn(hc, 64, 3, 3, generator=g) / 24.0
    b3 = torch.randn(hc, generator=g) * 0.1
    w1 = torch.randn(n2, hc, 1, 1, generator=g) / hc ** 0.5
    b1 = torch.randn(n2, generator=g)
    ref = F.conv2d(F.relu(F.conv2d(x, w3, b3, 1, 1)), w1, b1)
    if act2 == 2:
        ref = torch.sigmoid(ref)
    wp3 = ops.pack_conv_weight(w3.cuda())
    u = (ops.pack_wino24_weight if w24 else ops.pack_wino_weight)(wp3, 64, hc)
    sc, sh = ops.fold_bn(hc, None, b3.cuda())
    out = torch.full((B, n2, H, W), float("nan"), device="cuda")
    la = ops.head3x3_1x1_launch(_nhwc(x), u, sc, sh, w1.reshape(n2, hc).contiguous().cuda(), b1.cuda(), out, hc=hc, act2=act2, wino24=w24)
    la.run()
    assert la.kernel.startswith("head_wino24_kernel" if w24 else "conv3x3_wino_vs64_kernel")
    _close(out, ref, 2e-5 if act2 == 2 else 1e-4)
    a = out.clone()
    la.run()
    assert torch.equal(a, out)             # fixed summation order: deterministic


@pytest.mark.parametrize("B,H,W,cin,cout,S,act", [(2, 16, 16, 128, 27, 2, 0), (1, 13, 19, 512, 27, 8, 0), (3, 8, 16, 256, 64, 4, 1),
                                                   (1, 32, 32, 96, 100, 3, 1)])
def test_conv3x3_winograd_split_c(B, H, W, cin, cout, S, act):
    """cp_conv_desc.ksplit: the Winograd kernel split over the input channels into raw partial outputs + cp_splitk_reduce_f32
    (fixed-order sum, folded BN / bias, activation) against torch-CPU; ragged tiles, uneven stage split (96 channels in 3),
    padded 27 -> 32 output channels; twice -> same bits; `ops.wino_ksplit` picks a legal factor for the DLA-34 offset convs."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + cin + S)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bn = _rand_bn(g, cout)
    ref = F.batch_norm(F.conv2d(x, w, None, 1, 1), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5)
    ref = F.relu(ref) if act else ref
    wp = ops.pack_conv_weight(w.cuda())
    ld = ops.round_up(cout, 16)
    u = ops.pack_wino_weight(wp, cin, ld)
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    ws = torch.full((S, B * H * W, ld), float("nan"), device="cuda")
    out = torch.full((B, H, W, ld + 4), float("nan"), device="cuda")
    n = sc.numel()
    la = ops.conv2d_launch([_nhwc(x)], wp, torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), ws, kh=3, kw=3, stride=1, pad=1,
                           cout=ld, wino=u, ksplit=S)
    lb = ops.splitk_reduce_launch(ws, sc, sh, out[..., :ld], cout=ld, act=ops.ACT_RELU if act else ops.ACT_NONE)
    la.run(); lb.run()
    first = out.clone()
    la.run(); lb.run()
    assert torch.equal(first[..., :ld], out[..., :ld]) and torch.isnan(out[..., ld:]).all() and not torch.isnan(ws).any()
    _close(out[..., :cout].permute(0, 3, 1, 2), ref, 1e-4)
    for (b_, h_, c_) in ((16, 16, 512), (16, 32, 256), (16, 64, 128), (16, 128, 64), (1, 128, 64)):
        s_ = ops.wino_ksplit(b_, h_, h_, c_, 27)
        assert s_ >= 1 and (c_ // 16) // s_ >= 4 or s_ == 1


def test_conv3x3_winograd_fuzz_vs_direct_kernel():
    """Seeded random shapes (odd H/W, batch 1..3, ragged channel tiles, strided input / output / residual views, every
    activation, every block shape): the Winograd kernel against the direct halo-patch kernel on the same buffers."""
    from centerpose_amd import ops
    rng = np.random.RandomState(5)
    g = torch.Generator().manual_seed(5)
    variants = [0, 11, 12, 21]
    for it in range(14):
        B = int(rng.randint(1, 4))
        H, W = int(rng.randint(3, 41)), int(rng.randint(3, 45))
        cin = int(rng.choice([32, 48, 64, 96]))
        cout = int(rng.choice([16, 27, 32, 40, 64, 100, 128]))
        act = int(rng.choice([ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID]))
        var = 6400 + int(rng.randint(0, 3)) if (cin == 64 and it % 3 == 0) else int(variants[it % len(variants)])
        in_ld, out_ld = cin + 16 * int(rng.randint(0, 2)), ops.round_up(cout, 4) + 4 * int(rng.randint(0, 3))
        xb = torch.randn(B, H, W, in_ld, generator=g).cuda()
        x = xb[..., in_ld - cin:]                                         # channel-offset view
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).cuda()
        wp = ops.pack_conv_weight(w)
        u = ops.pack_wino_weight(wp, cin, cout)
        sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in _rand_bn(g, cout)))
        use_res = bool(rng.randint(0, 2))
        resb = torch.randn(B, H, W, out_ld, generator=g).cuda() if use_res else None
        res = resb[..., :cout] if use_res else None
        outs = []
        for wino in (None, u):
            ob = torch.full((B, H, W, out_ld), float("nan"), device="cuda")
            ops.conv2d([x], wp, sc, sh, ob[..., :cout], kh=3, kw=3, stride=1, pad=1, cout=cout, act=act, res=res,
                       tile=var if wino is not None else 0, wino=wino)
            assert torch.isnan(ob[..., cout:]).all(), "case %d wrote past Cout" % it
            outs.append(ob[..., :cout])
        _close(outs[1], outs[0], 1e-4)


@pytest.mark.parametrize("cin,cout,k,stride,pad,hw,S", [(512, 512, 3, 2, 1, (13, 10), 2), (2048, 512, 1, 1, 0, (6, 5), 4), (256, 128, 3, 2, 1, (9, 9), 3),
                                                        (64, 64, 1, 1, 0, (7, 9), 4), (48, 192, 3, 2, 1, (8, 8), 27)])
def test_conv2d_split_k(cin, cout, k, stride, pad, hw, S):
    """cp_conv_desc.ksplit on the generic implicit-GEMM kernel (round 4: res_50 layer4's small-M launches): splits that start in
    the middle of a tap, ragged M, the extreme S = K / 16 (one k-step per block); raw partial sums + cp_splitk_reduce_f32 (folded
    BN + ReLU) == the unsplit launch within fp32 re-association and == torch-CPU; twice -> same bits."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cin + cout + S)
    B, (H, W) = 2, hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bn = _rand_bn(g, cout)
    ref = F.relu(_ref_bn(F.conv2d(x, w, None, stride, pad), bn))
    Ho, Wo = ref.shape[2], ref.shape[3]
    wp = ops.pack_conv_weight(w.cuda())
    ldw = wp.shape[0]
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    ws = torch.full((S, B * Ho * Wo, ldw), float("nan"), device="cuda")
    out = torch.full((B, Ho, Wo, cout), float("nan"), device="cuda")
    la = ops.conv2d_launch([_nhwc(x)], wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, kh=k, kw=k, stride=stride,
                           pad=pad, cout=ldw, ksplit=S)
    lb = ops.splitk_reduce_launch(ws, sc, sh, out, cout=cout, act=ops.ACT_RELU)
    la.run(); lb.run()
    first = out.clone()
    la.run(); lb.run()
    # ("igemm_bf16x3_kernel" when the suite runs with the opt-in CP_SPLIT_BF16=1: same test, same tolerances)
    assert torch.equal(first, out) and la.kernel.startswith(("igemm_conv_kernel", "igemm_bf16x3_kernel"))
    _close(out.permute(0, 3, 1, 2), ref)
    whole = torch.empty(B, Ho, Wo, cout, device="cuda")
    ops.conv2d([_nhwc(x)], wp, sc, sh, whole, kh=k, kw=k, stride=stride, pad=pad, cout=cout, act=ops.ACT_RELU)
    _close(out, whole, 1e-5)
    assert ops.conv_ksplit(8 * 16 * 16, 512, 9 * 512) == 2 and ops.conv_ksplit(8 * 16 * 16, 512, 2048) == 2      # res_50 B = 8 layer4
    assert ops.conv_ksplit(16 * 64 * 64, 128, 9 * 64) == 1 and ops.conv_ksplit(8 * 16 * 16, 512, 128) == 1         # enough blocks / K too short


@pytest.mark.parametrize("cin,cout,hw,B", [(32, 32, (16, 16), 1), (64, 64, (20, 28), 3), (32, 27, (19, 16), 2), (48, 128, (9, 35), 2),
                                           (128, 192, (16, 16), 2), (256, 96, (8, 8), 2), (128, 128, (64, 64), 2), (16, 40, (33, 17), 1),
                                           (512, 64, (16, 16), 1)])
def test_conv3x3_winograd24_kernel(cin, cout, hw, B):
    """fused Winograd F(2x4,3x3) kernel (conv3x3_wino24.hip, cp_conv_desc.tile = 24): odd sizes, ragged 16x16 tiles, residual,
    ragged channel tiles, scalar-store tail, long channel loops; against the torch-CPU fp32 direct convolution at the same
    2e-4 * max|ref| as the F(2x2) kernel (F(4,3)'s larger transform constants cost about one digit: ~1e-5 measured)."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(11 * cin + cout)
    H, W = hw
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bn = _rand_bn(g, cout)
    res = torch.randn(B, cout, H, W, generator=g) if cout != 96 else None
    y = _ref_bn(F.conv2d(x, w, None, 1, 1), bn)
    ref = F.relu(y + res) if res is not None else y
    wp = ops.pack_conv_weight(w.cuda())
    u = ops.pack_wino24_weight(wp, cin, cout)
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    ld = 32 if cout == 27 else cout
    buf = torch.full((B, H, W, ld), float("nan"), device="cuda")
    out = buf[..., :cout]
    resn = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    la = ops.conv2d_launch([_nhwc(x)], wp, sc, sh, out, kh=3, kw=3, stride=1, pad=1, cout=cout,
                           act=ops.ACT_RELU if res is not None else ops.ACT_NONE, res=resn, tile=ops.WINO24, wino=u)
    la.run()
    assert la.kernel in ("conv3x3_wino24_kernel<true>", "conv3x3_wino24_kernel<false>")     # the name rocprofv3 prints
    _close(out.permute(0, 3, 1, 2), ref)
    if ld != cout:
        assert torch.isnan(buf[..., cout:]).all()      # nothing stored past Cout
    first = out.clone()
    la.run()
    assert torch.equal(first, out)


def test_conv3x3_winograd24_group_launch():
    """cp_conv3x3_winograd24_group_f32: independent convolutions of different shapes (HRNet's branches: 32 ch on the large map ... 256 ch
    on the small one) in ONE launch, outputs views of one storage; every member == its own single launch bit for bit (same kernel body,
    same per-output arithmetic) and == torch-CPU; 2, 3 and 4 members, with / without residual, ragged maps."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(44)
    shapes = [(32, (40, 24)), (64, (20, 12)), (128, (10, 6)), (256, (5, 3))]
    B = 2
    for nm in (2, 3, 4):
        sizes = [B * h * w * c for c, (h, w) in shapes[:nm]]
        whole = torch.full((sum(sizes),), float("nan"), device="cuda")
        members, refs, singles, off = [], [], [], 0
        for i, (c, (h, w)) in enumerate(shapes[:nm]):
            x = torch.randn(B, c, h, w, generator=g)
            wt = torch.randn(c, c, 3, 3, generator=g) / (c * 9) ** 0.5
            bn = _rand_bn(g, c)
            res = torch.randn(B, c, h, w, generator=g) if i % 2 == 0 else None
            y = _ref_bn(F.conv2d(x, wt, None, 1, 1), bn)
            refs.append(F.relu(y + res) if res is not None else F.relu(y))
            wp = ops.pack_conv_weight(wt.cuda())
            u = ops.pack_wino24_weight(wp, c, c)
            sc, sh = ops.fold_bn(c, tuple(t.cuda() for t in bn))
            out = whole[off:off + sizes[i]].view(B, h, w, c)
            off += sizes[i]
            resn = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
            members.append(dict(x=_nhwc(x), wp=wp, u24=u, scale=sc, shift=sh, out=out, cout=c, act=ops.ACT_RELU, res=resn))
            single = torch.empty(B, h, w, c, device="cuda")
            ops.conv2d([members[-1]["x"]], wp, sc, sh, single, kh=3, kw=3, stride=1, pad=1, cout=c, act=ops.ACT_RELU, res=resn, wino=u,
                       tile=ops.WINO24)
            singles.append(single)
        la = ops.conv3x3_group_launch(members, whole)
        la.run()
        assert la.kernel.split("<")[0] == "conv3x3_wino24_group_kernel" and not torch.isnan(whole).any()
        for mm, single, ref in zip(members, singles, refs):
            assert torch.equal(mm["out"], single)
            _close(mm["out"].permute(0, 3, 1, 2), ref)


def test_conv3x3_winograd24_fuzz_vs_direct_kernel():
    """Seeded random shapes (odd H/W, ragged channel tiles, strided input / output / residual views, every activation): the
    F(2x4) kernel against the direct halo-patch kernel on the same buffers."""
    from centerpose_amd import ops
    rng = np.random.RandomState(24)
    g = torch.Generator().manual_seed(24)
    for it in range(12):
        B = int(rng.randint(1, 4))
        H, W = int(rng.randint(3, 41)), int(rng.randint(3, 45))
        cin = int(rng.choice([32, 48, 64, 96]))
        cout = int(rng.choice([16, 27, 32, 40, 64, 100, 128]))
        act = int(rng.choice([ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID]))
        in_ld, out_ld = cin + 16 * int(rng.randint(0, 2)), ops.round_up(cout, 4) + 4 * int(rng.randint(0, 3))
        xb = torch.randn(B, H, W, in_ld, generator=g).cuda()
        x = xb[..., in_ld - cin:]
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).cuda()
        wp = ops.pack_conv_weight(w)
        u = ops.pack_wino24_weight(wp, cin, cout)
        sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in _rand_bn(g, cout)))
        use_res = bool(rng.randint(0, 2))
        resb = torch.randn(B, H, W, out_ld, generator=g).cuda() if use_res else None
        res = resb[..., :cout] if use_res else None
        outs = []
        for wino in (None, u):
            ob = torch.full((B, H, W, out_ld), float("nan"), device="cuda")
            ops.conv2d([x], wp, sc, sh, ob[..., :cout], kh=3, kw=3, stride=1, pad=1, cout=cout, act=act, res=res,
                       tile=ops.WINO24 if wino is not None else 0, wino=wino)
            assert torch.isnan(ob[..., cout:]).all(), "case %d wrote past Cout" % it
            outs.append(ob[..., :cout])
        _close(outs[1], outs[0], 1e-4)


@pytest.mark.parametrize("cout,s,hw", [(16, 1, (40, 72)), (64, 2, (37, 70)), (16, 1, (512, 512)), (64, 2, (128, 96)), (16, 1, (37, 52)),
                                       (16, 1, (13, 50)), (16, 1, (3, 4)), (16, 1, (70, 200)), (64, 2, (512, 512)), (64, 2, (61, 132)),
                                       (64, 2, (5, 8)), (64, 1, (20, 24)), (16, 2, (20, 24))])
def test_stem7x7_kernel(cout, s, hw):
    """dedicated 7x7 stem (pose_dla_dcn.py:228-232 / msra_resnet.py:118-121) vs torch-CPU."""
    from centerpose_amd import ops
    g = torch.Generator().manual_seed(cout + s)
    x = torch.randn(2, 3, *hw, generator=g)
    w = torch.randn(cout, 3, 7, 7, generator=g) * 0.1
    bn = _rand_bn(g, cout)
    ref = F.relu(_ref_bn(F.conv2d(x, w, None, s, 3), bn))
    sc, sh = ops.fold_bn(cout, tuple(t.cuda() for t in bn))
    out = torch.full((2, ref.shape[2], ref.shape[3], cout), float("nan"), device="cuda")
    ops.stem7x7(x.cuda(), ops.pack_stem7_weight(w.cuda()), sc, sh, out, s)
    from centerpose_amd import _lib
    # 16 outputs / stride 1 (DLA) and 64 / stride 2 (ResNet) with whole float4 quads per row: the persistent weights-in-registers kernel;
    # everything else the LDS-weights one
    assert _lib.lib().cp_last_kernel().decode().startswith("stem7x7_c16_kernel" if (cout, s) in ((16, 1), (64, 2)) and hw[1] % 4 == 0 else "stem7x7_kernel<")
    _close(out.permute(0, 3, 1, 2), ref)
