"""What the face tests share on the library's side: the rule record, the calls of the HOST twins (cp_face_*_host) over the forms of
tests/draw_ref.py, and a float64 statement of ONE generic convolution launch record.

tests/layer_oracle.py states a plan hook by hook; its hooks do not include PRNet's given-output-size convolutions (`emit_conv_same`),
so the face tests carry `conv_launch_f64`: what a `cp_conv2d_f32` record computes, read from the record alone (descriptor, packed
weights, scale / shift, residual) and evaluated by torch in float64.  Tolerance rule of a launch (`conv_launch_tol`): a float32 dot
product of K terms accumulated in any order is within K * 2^-24 * sum |x_i w_i| of the exact one; the epilogue adds a handful of
roundings of the value itself.  So |error| <= (K + 16) * 2^-24 * (|scale| * conv(|x|, |w|) + |shift| + |res|) per element; behind a
sigmoid (slope <= 1/4) a quarter of that plus 1e-6 for the epilogue's exp and reciprocal (a few ulps of a value below 1)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import draw_util
import face_ref
import yuv_ref

GUARD = 257          # floats behind every output buffer that no call may touch
VP = ctypes.c_void_p
RULE = np.dtype([("vis_thresh", "<f4"), ("expand", "<f4"), ("min_size", "<i4"), ("boxes", "<i4")])
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def rule_struct(boxes, vis_thresh=face_ref.VIS, expand=1.6, min_size=1):
    rec = np.zeros(1, RULE)
    rec["vis_thresh"], rec["expand"], rec["min_size"], rec["boxes"] = vis_thresh, expand, min_size, int(boxes)
    return rec


def is_yuv(forms):
    return forms[0]["color"] not in ("bgr", "rgb")


def host_select(L, cand, boxes, cap, **rule):
    """-> (rc, slots [cap], counts [N], xform [cap, 3]); the arrays start as sentinels and carry a guard behind them."""
    N, M = cand.shape[:2]
    cand = np.ascontiguousarray(cand, np.float32)
    slots, counts = np.full(max(cap, 1) + GUARD, -7, np.int32), np.full(max(N, 1) + GUARD, -7, np.int32)
    xform = np.full(3 * max(cap, 1) + GUARD, np.nan, np.float32)
    rc = L.cp_face_select_host(N, cand.ctypes.data_as(VP), M, rule_struct(boxes, **rule).ctypes.data_as(VP), cap, slots.ctypes.data_as(VP),
                               counts.ctypes.data_as(VP), xform.ctypes.data_as(VP))
    assert (slots[max(cap, 1):] == -7).all() and (counts[max(N, 1):] == -7).all() and np.isnan(xform[3 * max(cap, 1):]).all()
    return rc, slots[:cap], counts[:N], xform[:3 * cap].reshape(cap, 3)


def host_crop(L, forms, M, slots, xform, matrix="bt601", table=None):
    """-> (rc, out float32 [cap * 3 * 256 * 256 + GUARD], NaN-filled before the call)."""
    cap = len(slots)
    table = draw_util.table_of(forms, [f["buf"].ctypes.data for f in forms]) if table is None else table
    slots, xform = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(xform, np.float32)
    out = np.full(cap * 3 * 256 * 256 + GUARD, np.nan, np.float32)
    if is_yuv(forms):
        coef = (ctypes.c_int * 6)(*yuv_ref.COEF[matrix])
        rc = L.cp_face_crop_yuv_frames_host(table.ctypes.data_as(VP), len(forms), coef, M, slots.ctypes.data_as(VP), xform.ctypes.data_as(VP), cap,
                                            out.ctypes.data_as(VP))
    else:
        rc = L.cp_face_crop_frames_host(table.ctypes.data_as(VP), len(forms), M, slots.ctypes.data_as(VP), xform.ctypes.data_as(VP), cap,
                                        out.ctypes.data_as(VP))
    return rc, out


def host_restore(L, net, slots, xform, uv, positions=True):
    """-> (rc, pos [cap, 256, 256, 3] or None, landmarks [cap, 68, 3]), guards checked."""
    cap = len(slots)
    net, slots = np.ascontiguousarray(net, np.float32), np.ascontiguousarray(slots, np.int32)
    xform, uv = np.ascontiguousarray(xform, np.float32), np.ascontiguousarray(uv, np.int32)
    pos = np.full(cap * 256 * 256 * 3 + GUARD, np.nan, np.float32) if positions else None
    lm = np.full(cap * 68 * 3 + GUARD, np.nan, np.float32)
    rc = L.cp_face_restore_host(net.ctypes.data_as(VP), slots.ctypes.data_as(VP), xform.ctypes.data_as(VP), cap, uv.ctypes.data_as(VP),
                                pos.ctypes.data_as(VP) if positions else None, lm.ctypes.data_as(VP))
    assert np.isnan(lm[cap * 68 * 3:]).all() and (pos is None or np.isnan(pos[cap * 256 * 256 * 3:]).all())
    return rc, (pos[:cap * 256 * 256 * 3].reshape(cap, 256, 256, 3) if positions else None), lm[:cap * 68 * 3].reshape(cap, 68, 3)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def uv_table(seed=5):
    """A [2, 68] table of cells that reaches the corners and the borders of the map."""
    r = np.random.RandomState(seed)
    uv = r.randint(0, 256, (2, 68)).astype(np.int32)
    uv[:, 0], uv[:, 1], uv[:, 2], uv[:, 3] = (0, 0), (255, 255), (0, 255), (255, 0)
    return uv


# ---- one convolution launch record in float64 -------------------------------------------------------------------------------------
def _conv_terms(l, get, dtype):
    """-> per sub-convolution (y [B, ldw, Ho, Wo] before scale / shift, the same over absolute values, sub index); `get(t)` gives the
    values of the record's tensor t as a CPU tensor of its shape."""
    d = l.desc
    assert l.fn == "cp_conv2d_f32" and d.ksplit <= 1 and d.tile == 0
    nsub = max(1, d.nsub)
    wp = get(l.tensors[4]).to(dtype).view(nsub, d.ldw, d.K)
    if d.inNCHW:
        x = get(l.tensors[0]).to(dtype)
        C = d.srcC[0]
        w = wp[:, :, :C * d.kh * d.kw].reshape(nsub, d.ldw, C, d.kh, d.kw)
    else:
        x = torch.cat([get(l.tensors[i]).to(dtype)[..., :d.srcC[i]] for i in range(d.nsrc)], -1).permute(0, 3, 1, 2)
        w = wp.view(nsub, d.ldw, d.kh, d.kw, x.shape[1]).permute(0, 1, 4, 2, 3)
    assert tuple(x.shape) == (d.B, x.shape[1], d.H, d.W)
    for sub in range(nsub):
        py, px = d.py - (sub >> 1 if nsub > 1 else 0), d.px - (sub & 1 if nsub > 1 else 0)
        pay, pax = (d.Ho - 1) * d.sy + d.kh - d.H - py, (d.Wo - 1) * d.sx + d.kw - d.W - px      # what the gather zero-fills behind the map
        xp = F.pad(x, (px, pax, py, pay))
        yield F.conv2d(xp, w[sub], None, (d.sy, d.sx)), F.conv2d(xp.abs(), w[sub].abs(), None, (d.sy, d.sx)), sub


def conv_launch_f64(l, get, dtype=torch.float64):
    """The record's output values and per-element tolerance -> (out, tol), both shaped like the record's output tensor; elements the
    launch does not write are NaN in `out`."""
    d = l.desc
    nsub = max(1, d.nsub)
    scale, shift = get(l.tensors[5]).to(dtype).view(1, -1, 1, 1), get(l.tensors[6]).to(dtype).view(1, -1, 1, 1)
    res = get(l.tensors[7]).to(dtype) if l.tensors[7] is not None else None
    shape = tuple(l.tensors[8].shape)
    out, tol = torch.full(shape, float("nan"), dtype=dtype), torch.zeros(shape, dtype=dtype)
    gamma = (d.K + 16) * 2.0 ** -24
    for y, ya, sub in _conv_terms(l, get, dtype):
        v, va = y * scale + shift, ya * scale.abs() + shift.abs()
        ooy, oox = (sub >> 1, sub & 1) if nsub > 1 else (d.ooy, d.oox)
        if res is not None:
            r = res[:, ooy::d.osy, oox::d.osx][:, :d.Ho, :d.Wo, :d.ldw].permute(0, 3, 1, 2)
            v[:, :r.shape[1]] += r
            va[:, :r.shape[1]] += r.abs()
        t = gamma * va
        if d.act == ACT_RELU:
            v = v.clamp_min(0)
        elif d.act == ACT_SIGMOID:
            v, t = torch.sigmoid(v), 0.25 * t + 1e-6
        else:
            assert d.act == ACT_NONE
        v, t = v[:, :d.Cout], t[:, :d.Cout]
        if d.outNCHW:
            out[:, :d.Cout, ooy::d.osy, oox::d.osx][:, :, :d.Ho, :d.Wo] = v
            tol[:, :d.Cout, ooy::d.osy, oox::d.osx][:, :, :d.Ho, :d.Wo] = t
        else:
            out[:, ooy::d.osy, oox::d.osx][:, :d.Ho, :d.Wo, :d.Cout] = v.permute(0, 2, 3, 1)
            tol[:, ooy::d.osy, oox::d.osx][:, :d.Ho, :d.Wo, :d.Cout] = t.permute(0, 2, 3, 1)
    return out, tol


class Shadow:
    """float64 shadows of the storages a plan's records name: `get(t)` views the shadow like t views its storage (a constant's shadow
    starts as its float32 values), `put(t, v)` writes v where t lies.  Running the records in order through `conv_launch_f64` with
    these is the plan evaluated in float64, buffer re-use included."""

    def __init__(self, dtype=torch.float64):
        self.dtype, self.store = dtype, {}

    def _whole(self, t):
        key = t.untyped_storage().data_ptr()
        if key not in self.store:
            flat = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
            self.store[key] = flat.detach().cpu().to(self.dtype)
        return self.store[key]

    def get(self, t):
        return torch.as_strided(self._whole(t), tuple(t.shape), tuple(t.stride()), t.storage_offset())

    def put(self, t, v):
        view = self.get(t)
        mask = ~torch.isnan(v)
        view[mask] = v[mask]


def run_plan_f64(launches, inp, x):
    """The records of a PRNet plan evaluated in float64 on input x [B, 3, H, W] -> the last record's output."""
    sh = Shadow()
    sh.put(inp, x.to(torch.float64))
    out = None
    for _, _, _, l in launches:
        v, _ = conv_launch_f64(l, sh.get)
        sh.put(l.out, v)
        out = sh.get(l.out)
    return out
