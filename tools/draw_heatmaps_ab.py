"""Same-process A/B of blending the joint heat maps over device frames against not drawing them and against what a caller had to do
for that picture without draw_heatmaps:

  (a) pre_process_batch(frames) + process(x)                                           the staged form of a detector run
  (b) (a) + draw_heatmaps(frames, hm_hp, metas)                                        csrc/draw_heat.hip, two launches
  (c) (a) + maps and frames to the host, the host painter cp_draw_heat_frames_host / cp_draw_heat_yuv_frames_host, frames back to
      the device: the round trip through the host that (b) removes.

Frames: random bytes as contiguous BGR [H,W,3] tensors or NV12 surfaces [H*3/2, W], on the device before any timing; dla_34 preset as
shipped, hm_hp = outputs[4] (its [0::2] view under FLIP_TEST: the images, not the twins).  (b) and (c) must leave the same bytes in
the frames; that is asserted first.  Every path is warmed, then timed for at least --seconds of work per round; five or more rounds
alternate the order of the paths so drift hits them alike.  Per path: wall ms per call as min / median over rounds and the spread
(max - min) / median; (b) - (a) and (c) - (a) from the medians.  Per configuration the floor of the blend launch is printed: the frame
bytes it must read plus the bytes it must write, at the 6.3 TB/s a streaming copy reaches on an MI355X.
--trace-pass: only path (b), 20 calls per kind at 480 x 640, N = 8 -- the run to put under rocprofv3 --kernel-trace --stats, whose
kernel times of draw_heat_colormap_kernel and draw_heat_blend_kernel<...> go beside that floor.
usage: python tools/draw_heatmaps_ab.py [--sizes 480x640] [--batches 1,8] [--kinds nv12,bgr] [--rounds 5] [--seconds 0.5]"""
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

STREAM_TBS = 6.3


def device_frames(kind, n, H, W, seed):
    r = np.random.RandomState(seed)
    shape = (H, W, 3) if kind == "bgr" else (H * 3 // 2, W)
    return [torch.from_numpy(r.randint(0, 256, shape).astype(np.uint8)).cuda() for _ in range(n)]


def floor_us(kind, N, H, W):
    """Frame bytes read plus written by one call, and the time a streaming copy needs for them."""
    nbytes = 2 * N * H * W * 3 if kind == "bgr" else 2 * N * (H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2))
    return nbytes, nbytes / (STREAM_TBS * 1e12) * 1e6


class HostRoundTrip:
    """Path (c): what a caller without draw_heatmaps does with the maps of process() and the frames."""

    def __init__(self, det, kind):
        from centerpose_amd import _lib, detector, draw
        self.det, self.kind, self.detector, self.draw, self.L = det, kind, detector, draw, _lib.lib()

    def __call__(self, frames, maps, metas):
        d, vp, ll = self.detector, ctypes.c_void_p, ctypes.c_longlong
        maps_h = np.ascontiguousarray(maps.cpu().numpy())
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
            new_h, new_w = self.det.input_geometry(H, W, 1)[0:2]
            t["mi"] = self.draw.heat_transform(metas[n], H, W, new_h, new_w)
        N, C, h, w = maps_h.shape
        style = self.draw.HeatmapStyle().struct(C)
        fn = self.L.cp_draw_heat_yuv_frames_host if self.kind == "nv12" else self.L.cp_draw_heat_frames_host
        rc = fn(table.ctypes.data_as(vp), N, maps_h.ctypes.data_as(vp), *(ll(s // 4) for s in maps_h.strides), C, h, w, style.ctypes.data_as(vp),
                *((0,) if self.kind == "nv12" else ()))
        assert rc == 0, self.L.cp_last_error()
        for f, h in zip(frames, hosts):
            f.copy_(torch.from_numpy(h))


def ab(det, kind, H, W, N, a):
    kw = dict(color=kind)
    flip = bool(det.cfg.TEST.FLIP_TEST)
    sets = [device_frames(kind, N, H, W, 300 + i) for i in range(2)]
    pristine = [[f.clone() for f in fs] for fs in sets]
    host_trip = HostRoundTrip(det, kind)
    torch.cuda.synchronize()

    def restore(i):
        for f, p in zip(sets[i], pristine[i]):
            f.copy_(p)

    def staged(i):
        x, metas = det.pre_process_batch(sets[i & 1], 1, **kw)
        outputs, dets = det.process(x)
        return (outputs[4][0::2] if flip else outputs[4]), metas, dets

    def path_a(i):
        return staged(i)[2]

    def path_b(i):
        hm_hp, metas, dets = staged(i)
        det.draw_heatmaps(sets[i & 1], hm_hp, metas, **kw)
        return dets

    def path_c(i):
        hm_hp, metas, dets = staged(i)
        host_trip(sets[i & 1], hm_hp, metas)
        return dets

    # (b) and (c) paint the same picture from the same maps
    for i in range(2):
        path_b(i)
        painted = [f.clone() for f in sets[i]]
        restore(i)
        path_c(i)
        assert all(torch.equal(p, f) for p, f in zip(painted, sets[i])), "(b) and (c) left different frames"
        assert not any(torch.equal(p, f) for p, f in zip(pristine[i], sets[i]))
        restore(i)
    nbytes, floor = floor_us(kind, N, H, W)
    # every timed call re-reads the frames as the last painting call left them: all three paths see the same frames
    if a.trace_pass:
        for i in range(20):
            path_b(i)
        torch.cuda.synchronize()
        print("%-4s %4dx%-4d N=%-3d blend floor: %d frame bytes read + written, %.2f us at %.1f TB/s" % (kind, H, W, N, nbytes, floor, STREAM_TBS),
              flush=True)
        return {"kind": kind, "size": [H, W], "N": N, "calls": 20, "frame_bytes": nbytes, "floor_us": round(floor, 3)}
    paths = {"a": ("(a) pre_process_batch + process", path_a), "b": ("(b) (a) + draw_heatmaps(hm_hp)", path_b),
             "c": ("(c) (a) + host heat-map round trip", path_c)}
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
        print("%-4s %4dx%-4d N=%-3d %-38s min %8.3f  median %8.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (kind, H, W, N, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+8.3f" % extra, steps[k],
                 len(ms[k])), flush=True)
    print("%-4s %4dx%-4d N=%-3d blend floor: %d frame bytes read + written, %.2f us at %.1f TB/s" % (kind, H, W, N, nbytes, floor, STREAM_TBS),
          flush=True)
    return {"kind": kind, "size": [H, W], "N": N, "frame_bytes": nbytes, "floor_us": round(floor, 3), "paths": res}


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
                except (_lib.CenterposeHipError, ValueError) as e:      # a batch the network itself refuses is reported, not hidden
                    print("%-4s %4dx%-4d N=%-3d not run: %s" % (kind, H, W, N, e), flush=True)
                    out.append({"kind": kind, "size": [H, W], "N": N, "not_run": str(e)})
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "flip_test": bool(det.cfg.TEST.FLIP_TEST), "configs": out}))


if __name__ == "__main__":
    main()
