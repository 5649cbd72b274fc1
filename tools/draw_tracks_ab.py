"""Same-process A/B of painting the tracker's result onto the frames of run_batch on the device against what a caller had to do without
draw="tracks":

  (a) run_batch(frames, return_device=True, embed=ex, track=trk)                 detection, embeddings, identities: nothing is painted
  (b) run_batch(frames, return_device=True, embed=ex, track=trk, draw="tracks")  the same, then the poses in identity colours
      (cp_track_row_ids, csrc/draw_results.hip) and the boxes and labels (csrc/draw_tracks.hip), in place on the device
  (c) (a), then frames, rows and slots to the host, the ids scattered in NumPy from trk.assignments, the host painters
      cp_draw_rows_ids_*_host and cp_draw_tracks_*_host, frames back to the device: the round trip through the host that (b) removes

Frames: pictures with large-scale structure as contiguous BGR [H,W,3] tensors or NV12 surfaces [H*3/2, W], on the device before any
timing; dla_34 preset as shipped (its own VIS_THRESH, default styles).  Every path owns a tracker and restores its frames from a device
copy before each call, so all three see the same frames in every call and every detection keeps matching its track.  (b) and (c) must
leave the same bytes in the frames; that is asserted over the first calls, until identities and labels are on the picture.  Every path
is warmed, then timed for at least --seconds of work per round; five or more rounds alternate the order of the paths so drift hits them
alike.  Per path: wall ms per call as min / median over rounds and the spread (max - min) / median; (b) - (a) and (c) - (a) from the
medians.
--trace-pass: only path (b), 20 calls per kind at N = 8 -- the run to put under rocprofv3 --kernel-trace --stats.
usage: python tools/draw_tracks_ab.py [--size 480x640] [--batches 1,4,8] [--kinds nv12,bgr] [--capacity 32] [--rounds 5] [--seconds 0.5]"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VP = ctypes.c_void_p


def device_frames(kind, n, H, W, seed):
    r = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        grid = torch.from_numpy(r.uniform(0, 255, (1, 3, 6, 8)))
        up = F.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
        img = np.clip(up + r.uniform(-20, 20, up.shape), 0, 255).astype(np.uint8)
        if kind == "bgr":
            out.append(torch.from_numpy(img.transpose(1, 2, 0).copy()).cuda())
        else:                                                  # luma from one channel, interleaved chroma from the other two at half size
            uv = np.stack([img[0, ::2, ::2], img[2, ::2, ::2]], -1).reshape(H // 2, W)
            out.append(torch.from_numpy(np.concatenate([img[1], uv], 0).copy()).cuda())
    return out


class HostRoundTrip:
    """Path (c): what a caller without draw="tracks" does after run_batch(return_device=True, embed=, track=)."""

    def __init__(self, det, kind):
        from centerpose_amd import _lib, detector, draw
        self.det, self.kind, self.detector, self.draw, self.L = det, kind, detector, draw, _lib.lib()
        self.yuv = kind == "nv12"
        self.matrix = "bt601" if self.yuv else None
        self.style = detector.DrawStyle().struct(self.matrix)
        self.tstyle = detector.TrackStyle()
        self.idp = draw._id_palette_struct(detector.TRACK_PALETTE, self.matrix)
        self.vis = float(det.cfg.TEST.VIS_THRESH)

    def __call__(self, frames, rows, res, tracks, trk):
        d = self.detector
        rows_h = np.ascontiguousarray(rows.cpu().numpy())
        slots = res.slots.cpu().numpy()
        N, M = rows_h.shape[:2]
        ids = np.full(N * M, -1, np.int32)
        flat = trk.assignments.reshape(-1)
        used = (slots[:flat.size] >= 0) & (flat >= 0)
        ids[slots[:flat.size][used]] = flat[used]
        hosts = [f.cpu().numpy() for f in frames]
        table = np.zeros(len(frames), d.YUV_FRAME_DESC if self.yuv else d.FRAME_DESC)
        for n, h in enumerate(hosts):
            t = table[n]
            if self.yuv:
                H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = d.yuv_frame_geometry([h.shape], [h.strides], "nv12")
                t["y_base"], t["y_row"], t["y_pix"], t["u_base"], t["v_base"], t["c_row"], t["c_pix"] = (
                    h.ctypes.data, y_row, y_pix, h.ctypes.data + u_off, h.ctypes.data + v_off, c_row, c_pix)
            else:
                H, W, row, pix, ch = d.frame_geometry(h.shape, h.strides)
                t["base"], t["row_stride"], t["pix_stride"], t["ch_off"] = h.ctypes.data, row, pix, ch
            t["H"], t["W"], t["NH"], t["NW"], t["mid_off"] = H, W, H, W, -1
        L = self.L
        fn = L.cp_draw_rows_ids_yuv_frames_host if self.yuv else L.cp_draw_rows_ids_frames_host
        rc = fn(table.ctypes.data_as(VP), N, rows_h.ctypes.data_as(VP), M, ctypes.c_float(self.vis), self.style.ctypes.data_as(VP),
                ids.ctypes.data_as(VP), self.idp.ctypes.data_as(VP))
        assert rc == 0, L.cp_last_error()
        items, counts = self.draw.track_items(tracks, self.tstyle, self.matrix)
        fn = L.cp_draw_tracks_yuv_frames_host if self.yuv else L.cp_draw_tracks_frames_host
        rc = fn(table.ctypes.data_as(VP), N, items.ctypes.data_as(VP), counts.ctypes.data_as(VP), items.shape[1], self.tstyle.box_thickness,
                self.tstyle.font_scale)
        assert rc == 0, L.cp_last_error()
        for f, h in zip(frames, hosts):
            f.copy_(torch.from_numpy(h))
        return rows


def ab(det, ex, kind, H, W, N, a):
    from centerpose_amd import track
    kw = dict(color=kind, return_device=True, embed=ex)
    pristine = device_frames(kind, N, H, W, 300)
    frames = {k: [p.clone() for p in pristine] for k in "abc"}
    host_trip = HostRoundTrip(det, kind)
    trk = {k: track.DeepSortTracker(a.capacity, streams=N) for k in "abc"}
    torch.cuda.synchronize()

    def restore(k):
        for f, p in zip(frames[k], pristine):
            f.copy_(p)

    def path_a():
        restore("a")
        return det.run_batch(frames["a"], track=trk["a"], **kw)

    def path_b():
        restore("b")
        return det.run_batch(frames["b"], track=trk["b"], draw="tracks", **kw)

    def path_c():
        restore("c")
        rows, res, tracks = det.run_batch(frames["c"], track=trk["c"], **kw)
        host_trip(frames["c"], rows, res, tracks, trk["c"])
        return rows, res, tracks

    # (b) and (c) paint the same picture, call after call, until identities and labels are on it
    labels = matched = live = 0
    for call in range(5):
        ra, rb, rc = path_a(), path_b(), path_c()
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[0], rc[0])
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(ra[2], rb[2], rc[2]))
        assert all(torch.equal(p, f) for p, f in zip(frames["b"], frames["c"])), "(b) and (c) left different frames"
        assert all(torch.equal(p, f) for p, f in zip(frames["a"], pristine))
        labels, matched = sum(len(t) for t in rb[2]), int((trk["b"].assignments >= 0).sum())
        live = int((ra[0][:, :, 4] > host_trip.vis).sum())
    if a.trace_pass:
        for _ in range(20):
            path_b()
        torch.cuda.synchronize()
        return {"kind": kind, "size": [H, W], "N": N, "calls": 20, "labels_per_call": labels}
    paths = {"a": ("(a) run_batch(embed, track)", path_a), "b": ("(b) run_batch(embed, track, draw=\"tracks\")", path_b),
             "c": ("(c) (a) + host painters round trip", path_c)}
    keys, steps = list("abc"), {}
    for k in keys:
        for _ in range(2):
            paths[k][1]()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            paths[k][1]()
        torch.cuda.synchronize()
        steps[k] = max(3, int(math.ceil(a.seconds / ((time.perf_counter() - t0) / 3))))
    ms = {k: [] for k in keys}
    for r in range(a.rounds):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps[k]):
                paths[k][1]()
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
        print("%-4s %4dx%-4d N=%-3d %-44s min %8.3f  median %8.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (kind, H, W, N, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+8.3f" % extra, steps[k],
                 len(ms[k])), flush=True)
    print("%-4s %4dx%-4d N=%-3d live rows %d, matched rows %d, labels %d per call" % (kind, H, W, N, live, matched, labels), flush=True)
    return {"kind": kind, "size": [H, W], "N": N, "live_rows": live, "matched_rows": matched, "labels": labels, "paths": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--kinds", default="nv12,bgr")
    ap.add_argument("--capacity", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--trace-pass", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    from centerpose_amd import _lib, config, detector, reid, synth
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    ex = reid.ReidExtractor(synth.make_state_dict("reid", seed=7), capacity=a.capacity)
    H, W = (int(v) for v in a.size.split("x"))
    batches = [8] if a.trace_pass else [int(n) for n in a.batches.split(",")]
    print("draw_tracks_ab: dla_34 as shipped, frames %dx%d, capacity %d; %d rounds of >= %.2f s per path" % (H, W, a.capacity, a.rounds, a.seconds),
          flush=True)
    out = []
    for kind in a.kinds.split(","):
        for N in batches:
            try:
                out.append(ab(det, ex, kind, H, W, N, a))
            except _lib.CenterposeHipError as e:               # a batch the network itself refuses is reported, not hidden
                print("%-4s %4dx%-4d N=%-3d not run: %s" % (kind, H, W, N, e), flush=True)
                out.append({"kind": kind, "size": [H, W], "N": N, "not_run": str(e)})
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "vis_thresh": float(det.cfg.TEST.VIS_THRESH), "configs": out}))


if __name__ == "__main__":
    main()
