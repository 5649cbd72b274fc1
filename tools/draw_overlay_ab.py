"""Same-process A/B of painting score labels and translucent limbs on the device against the default style and against what a caller
had to do for them without the overlay painters:

  (a) run_batch(frames, return_device=True, draw=True)                                  the default style: csrc/draw_results.hip
  (b) (a) with draw_style=DrawStyle(labels=True, limb_opacity=128)                      csrc/draw_overlay.hip
  (c) run_batch(frames, return_device=True), then frames and rows to the host, the host painter cp_draw_overlay_frames_host /
      cp_draw_overlay_yuv_frames_host with the style of (b), frames back to the device: the round trip through the host that (b)
      removes.  (c) does not pay (a)'s own painting, so (c) - (a) is that much too small.

Frames: random bytes as contiguous BGR [H,W,3] tensors or NV12 surfaces [H*3/2, W], on the device before any timing; dla_34 preset as
shipped (its own VIS_THRESH), so the rows are what that network gives for these frames -- the number of live rows per frame is
printed.  (b) and (c) must leave the same bytes in the frames; that is asserted first.  Every path is warmed, then timed for at least
--seconds of work per round; five or more rounds alternate the order of the paths so drift hits them alike.  Per path: wall ms per
call as min / median over rounds and the spread (max - min) / median; (b) - (a) and (c) - (a) from the medians.
--trace-pass: only path (b), 20 calls per kind at 480 x 640, N = 8 -- the run to put under rocprofv3 --kernel-trace --stats.
usage: python tools/draw_overlay_ab.py [--sizes 480x640] [--batches 1,8] [--kinds nv12,bgr] [--rounds 5] [--seconds 0.5]"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_frames(kind, n, H, W, seed):
    r = np.random.RandomState(seed)
    shape = (H, W, 3) if kind == "bgr" else (H * 3 // 2, W)
    return [torch.from_numpy(r.randint(0, 256, shape).astype(np.uint8)).cuda() for _ in range(n)]


class HostRoundTrip:
    """Path (c): what a caller without the overlay painters does after run_batch(return_device=True)."""

    def __init__(self, det, kind, style):
        from centerpose_amd import _lib, detector
        self.det, self.kind, self.detector, self.L = det, kind, detector, _lib.lib()
        matrix = "bt601" if kind == "nv12" else None
        self.style, self.overlay = style.struct(matrix), style.overlay_struct(matrix)
        self.vis = float(det.cfg.TEST.VIS_THRESH)

    def __call__(self, frames, rows):
        d, vp = self.detector, ctypes.c_void_p
        rows_h = np.ascontiguousarray(rows.cpu().numpy())
        hosts = [f.cpu().numpy() for f in frames]
        table = np.zeros(len(frames), d.YUV_FRAME_DESC if self.kind == "nv12" else d.FRAME_DESC)
        for n, h in enumerate(hosts):
            t = table[n]
            if self.kind == "nv12":
                H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = d.yuv_frame_geometry([h.shape], [h.strides], "nv12")
                t["y_base"], t["y_row"], t["y_pix"], t["u_base"], t["v_base"], t["c_row"], t["c_pix"] = (
                    h.ctypes.data, y_row, y_pix, h.ctypes.data + u_off, h.ctypes.data + v_off, c_row, c_pix)
            else:
                H, W, row, pix, ch = d.frame_geometry(h.shape, h.strides)
                t["base"], t["row_stride"], t["pix_stride"], t["ch_off"] = h.ctypes.data, row, pix, ch
            t["H"], t["W"], t["NH"], t["NW"], t["mid_off"] = H, W, H, W, -1
        fn = self.L.cp_draw_overlay_yuv_frames_host if self.kind == "nv12" else self.L.cp_draw_overlay_frames_host
        rc = fn(table.ctypes.data_as(vp), len(frames), rows_h.ctypes.data_as(vp), rows_h.shape[1], ctypes.c_float(self.vis),
                self.style.ctypes.data_as(vp), None, None, self.overlay.ctypes.data_as(vp))
        assert rc == 0, self.L.cp_last_error()
        for f, h in zip(frames, hosts):
            f.copy_(torch.from_numpy(h))
        return rows


def ab(det, kind, H, W, N, a):
    from centerpose_amd import detector
    kw = dict(color=kind)
    style = detector.DrawStyle(labels=True, limb_opacity=128)
    sets = [device_frames(kind, N, H, W, 300 + i) for i in range(2)]
    pristine = [[f.clone() for f in fs] for fs in sets]
    host_trip = HostRoundTrip(det, kind, style)
    torch.cuda.synchronize()

    def restore(i):
        for f, p in zip(sets[i], pristine[i]):
            f.copy_(p)

    def path_a(i):
        return det.run_batch(sets[i & 1], return_device=True, draw=True, **kw)

    def path_b(i):
        return det.run_batch(sets[i & 1], return_device=True, draw=True, draw_style=style, **kw)

    def path_c(i):
        return host_trip(sets[i & 1], det.run_batch(sets[i & 1], return_device=True, **kw))

    # (b) and (c) paint the same picture from the same rows
    live = 0
    for i in range(2):
        rows = path_b(i)
        live += int((rows[:, :, 4] > host_trip.vis).sum())
        painted = [f.clone() for f in sets[i]]
        restore(i)
        assert torch.equal(path_c(i), rows)
        assert all(torch.equal(p, f) for p, f in zip(painted, sets[i])), "(b) and (c) left different frames"
        assert not all(torch.equal(p, f) for p, f in zip(pristine[i], sets[i])) or live == 0
        restore(i)
    # every timed call re-reads the frames as the last painting call left them: all three paths see the same frames
    if a.trace_pass:
        for i in range(20):
            path_b(i)
        torch.cuda.synchronize()
        return {"kind": kind, "size": [H, W], "N": N, "calls": 20}
    paths = {"a": ("(a) run_batch(draw=True)", path_a), "b": ("(b) (a) with labels, limb_opacity=128", path_b),
             "c": ("(c) run_batch + host overlay round trip", path_c)}
    keys, steps = list("abc"), {}
    for k in keys:
        for i in range(2):
            paths[k][1](i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(3):
            paths[k][1](i)
        torch.cuda.synchronize()
        steps[k] = max(3, int(math.ceil(a.seconds / ((time.perf_counter() - t0) / 3))))
    ms = {k: [] for k in keys}
    for r in range(a.rounds):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps[k]):
                paths[k][1](i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    res = {}
    for k in keys:
        v, lo = med[k], min(ms[k])
        spread = 100.0 * (max(ms[k]) - lo) / v
        extra = None if k == "a" else v - med["a"]
        res[k] = {"path": paths[k][0], "ms_per_call_median": round(v, 4), "ms_per_call_min": round(lo, 4), "spread_pct": round(spread, 2),
                  "steps_per_round": steps[k], "minus_a_ms_per_call": None if extra is None else round(extra, 4),
                  "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-4s %4dx%-4d N=%-3d %-42s min %8.3f  median %8.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (kind, H, W, N, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+8.3f" % extra, steps[k],
                 len(ms[k])), flush=True)
    return {"kind": kind, "size": [H, W], "N": N, "live_rows_per_frame": live / (2.0 * N), "paths": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x640")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--kinds", default="nv12,bgr")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--trace-pass", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    from centerpose_amd import _lib, config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    batches = [int(n) for n in a.batches.split(",")]
    if a.trace_pass:
        sizes, batches = [(480, 640)], [8]
    out = []
    for kind in a.kinds.split(","):
        for (H, W) in sizes:
            for N in batches:
                try:
                    out.append(ab(det, kind, H, W, N, a))
                except _lib.CenterposeHipError as e:           # a batch the network itself refuses is reported, not hidden
                    print("%-4s %4dx%-4d N=%-3d not run: %s" % (kind, H, W, N, e), flush=True)
                    out.append({"kind": kind, "size": [H, W], "N": N, "not_run": str(e)})
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "vis_thresh": float(det.cfg.TEST.VIS_THRESH), "configs": out}))


if __name__ == "__main__":
    main()
