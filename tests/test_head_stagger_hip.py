"""The staggered form of `head_wino24_kernel` (waves 4-7 half a channel tile behind waves 0-3) against its lock-step form.

`CP_HEAD_STAGGER=0` selects the lock-step form, the default the staggered one (head_wino24.hip; read by the launcher on every call).
Both forms add the same numbers in the same order, so they must agree bit for bit; what can go wrong in the staggered form is the
lifetime of the two reduction buffers, which the two wave groups write half a tile apart.  Every launch is forced (`wino24=True`) at
the smallest shapes that still differ in that respect, all with 64 input channels:

* one block, 32 mid channels: ONE channel tile -- the stagger has no second tile and both groups fall straight into the last reduction;
* 64 mid channels: two tiles -- the first reuse of both buffers;
* 256 mid channels: eight tiles, the depth of the shipped heads;
* B = 2, 24 x 40: partial blocks on the right and the lower edge, halo zeros, several blocks;

each with n2 = 1, 2 (the kernels that have the staggered form), 17, 33, 34 (the second-MFMA-phase kernels, lock-step under either
setting), with and without the sigmoid.  Inputs are of mixed sign, and the ReLU between the two convolutions cuts.  Asserted per case:
the two settings report the same kernel name and `torch.equal` outputs; the default setting is inside the float64 oracle's bound
(tests/launch_oracle.py, its tolerance unchanged).  At one shape 20 launches in a row on one stream into 20 buffers give the same bits.
"""
import contextlib
import functools
import os

import pytest
import torch

import launch_oracle as L
import layer_oracle as lo

pytestmark = pytest.mark.gpu

SWITCH = "CP_HEAD_STAGGER"
SHAPES = {"1tile": (1, 16, 16, 32), "2tiles": (1, 16, 16, 64), "8tiles": (1, 16, 16, 256), "edges": (2, 24, 40, 64),      # B, H, W, hc
          "replay": (2, 24, 40, 256)}
CASES = [(s, n2, sig) for s in list(SHAPES)[:4] for n2 in (1, 2, 17, 33, 34) for sig in (False, True)]
IDS = ["%s-n%d%s" % (s, n2, "-sigmoid" if sig else "") for s, n2, sig in CASES]


@functools.lru_cache(maxsize=None)
def _case(shape, n2, sig):
    """launch_oracle.Case of one head branch: the weights of `launch_oracle.make_case`'s head rows, an input of mixed sign"""
    B, H, W, hc = SHAPES[shape]
    row = L._r("stagger-%s-n%d-%d" % (shape, n2, sig), "head", "wino24", "head_wino24_kernel" + L._head_inst(n2), B=B, H=H, W=W, cin=64, hc=hc,
               cout=n2, sigmoid=sig, wino24=True, res=False)
    g = torch.Generator().manual_seed(7000 + 100 * list(SHAPES).index(shape) + 2 * n2 + sig)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"h.0.weight": r(hc, 64, 3, 3) * (2.0 / (9 * 64)) ** 0.5 * lo.spread_factors(hc).view(-1, 1, 1, 1), "h.0.bias": r(hc) * 0.1,
          "h.2.weight": r(n2, hc, 1, 1) * (2.0 / hc) ** 0.5 * lo.spread_factors(n2).view(-1, 1, 1, 1),
          "h.2.bias": torch.full((n2,), L.SIGMOID_BIAS) if sig else r(n2) * 0.1}
    return L.Case(row, row.p, sd, r(B, 64, H, W), None, None, H, W, n2)


@contextlib.contextmanager
def _switch(value):
    """CP_HEAD_STAGGER = `value` (None: unset, the default) while the launches inside are enqueued"""
    old = os.environ.get(SWITCH)
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


@functools.lru_cache(maxsize=None)
def _run(shape, n2, sig, value):
    """-> (kernel name, logical NCHW result on the CPU, NaN guard intact) of one launch under CP_HEAD_STAGGER = `value`"""
    with torch.no_grad():
        (la,), read = L.build_launches(_case(shape, n2, sig))
        with _switch(value):
            la.run()
        torch.cuda.synchronize()
        _, out, guard = read()
    return la.kernel, out, guard


@pytest.mark.parametrize("shape,n2,sig", CASES, ids=IDS)
def test_staggered_form_is_bit_identical_to_lock_step(shape, n2, sig):
    k0, lock, g0 = _run(shape, n2, sig, "0")
    k1, stag, g1 = _run(shape, n2, sig, None)
    assert k0 == k1 == _case(shape, n2, sig).row.kernel
    assert g0 and g1, "stored outside the output (NaN guard overwritten)"
    assert not torch.isnan(lock).any() and not torch.isnan(stag).any()
    assert torch.equal(lock, stag), "first difference at %s" % (lo.first_unequal(stag, lock),)


@pytest.mark.parametrize("shape,n2,sig", CASES, ids=IDS)
def test_default_form_matches_fp64_reference(shape, n2, sig):
    case = _case(shape, n2, sig)
    _, out, _ = _run(shape, n2, sig, None)
    with torch.no_grad():
        o64 = L.evaluate(case, torch.float64)
    w, fails = L.check(case, out, None, o64)
    print("\n%-24s worst err / (u A) %.3f (c = %.1f) at %s" % (case.row.id, w.ratio, lo.c_for("wino24", o64.K), w.loc))
    assert not fails, "\n".join(fails)


def test_twenty_launches_in_a_row_give_the_same_bits():
    """B = 2, 24 x 40, 256 mid channels, n2 = 2: twelve blocks of eight tiles each, 20 launches back to back on one stream, each into its
    own buffer.  A barrier missing from the lifetime argument of the reduction buffers would show as a difference between them."""
    from centerpose_amd import ops
    case = _case("replay", 2, False)
    with torch.no_grad():
        (la,), _ = L.build_launches(case)
        outs = [torch.full_like(la.out, float("nan")) for _ in range(20)]
        las = [ops.Launch(la.fn, la.desc, la.tensors[:la.out_index] + [o], la.ints) for o in outs]
        with _switch(None):
            for l in las:
                l.run()
        torch.cuda.synchronize()
    assert {l.kernel for l in las} == {"head_wino24_kernel<2, 0>"}
    assert not torch.isnan(outs[0]).any()
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(o, outs[0]), "launch %d differs from launch 0 at %s" % (i, lo.first_unequal(o, outs[0]))
