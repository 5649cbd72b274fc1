"""Same-process A/B of the mesh rasteriser on the device against what a caller had to do without it:

  (a)  rows = run_batch(frames, return_device=True), then FaceAligner.align(frames, rows=rows)     detection and alignment on the device
  (b)  (a), then FaceRenderer.vertex_colors and two FaceRenderer.render calls: the depth image      + face_vertex_colors_kernel and twice
       (attrs=None) and the coloured rendering (attrs = the colours), in a 256 x 256 window per       the three render launches
       face                                                                                           (csrc/face_render.hip)
  (c)  (a), then the position maps and the frame to the host and, per face, get_colors and a VECTORISED NumPy renderer of the same rule
       (all triangles at once per box offset, the winner by np.maximum.at on the same 64-bit keys) -- not the reference's three nested
       Python loops, which take seconds per face

The plan runs on synthetic weights, whose maps are noise; a mesh over noise is triangles as large as the crop, nothing like a face.  So
every path, (a) included, overwrites the maps of its result with smooth stand-in maps (an ellipsoid cap about 180 px wide per face,
0.7 px per map cell: a triangle covers about one pixel, as on a real face; one device copy that all three paths pay).  The mesh is
grid_triangles over a 210 x 210 block of map cells: 44 100 vertices, 87 362 triangles (the reference's own: 43 867 and 86 906; the
product ships no reference data).  Frames: random bytes with large-scale structure, on the device before any timing; dla_34 preset as
shipped; the frames are such that all `capacity` slots are taken (asserted).  Before timing, (b)'s tri and images are compared with
(c)'s: equal, bit for bit.  Every path is warmed, then timed for at least --seconds of work per round; five or more rounds alternate
the order of the paths.  Per path: wall ms per call as min / median over rounds and the spread (max - min) / median; this - (a) from
the medians.  There is no pass mark.

  --kernels K   instead of the A/B: K vertex_colors + render(depth) + render(colours) calls on the stand-in maps and nothing else, for a
                kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/face_render_ab.py --kernels 20); prints the
                bytes of the floor: the key buffer written and read once plus the gathered vertices
usage: python tools/face_render_ab.py [--capacity 8] [--window 256] [--rounds 5] [--seconds 0.5]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BLOCK = 210


def stand_in_maps(cap, seed=21):
    """float32 [cap, 256, 256, 3]: per slot a smooth face-like surface in frame coordinates, and the centre (x, y) of each."""
    r = np.random.RandomState(seed)
    c, rr = np.meshgrid(np.arange(256.0) - 128.0, np.arange(256.0) - 128.0)
    maps, centres = [], []
    for s in range(cap):
        cx, cy = 150.0 + 45.0 * s + r.uniform(0, 1), 200.0 + 8.0 * s + r.uniform(0, 1)
        z = 70.0 * np.sqrt(np.maximum(0.0, 1.0 - (c / 150.0) ** 2 - (rr / 150.0) ** 2))
        m = np.stack([cx + 0.7 * c + 0.002 * z * c, cy + 0.75 * rr, z], -1) + r.uniform(-0.05, 0.05, (256, 256, 3))
        maps.append(m.astype(np.float32))
        centres.append((cx, cy))
    return np.stack(maps), np.asarray(centres)


def numpy_render(v32, tri, x0, y0, h, w, attrs):
    """The rule of csrc/face_render_arith.h for one face, vectorised over the triangles -> (tri int32 [h, w], image float32 [h, w, C])."""
    v = v32.astype(np.float64)
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    T = len(tri)
    d = ((p0[:, 2] + p1[:, 2] + p2[:, 2]) / 3.0).astype(np.float32) + np.float32(0.0)
    xs, ys = np.stack([p0[:, 0], p1[:, 0], p2[:, 0]]), np.stack([p0[:, 1], p1[:, 1], p2[:, 1]])
    umin, umax = np.maximum(np.ceil(xs.min(0)), x0), np.minimum(np.floor(xs.max(0)), x0 + w - 1)
    vmin, vmax = np.maximum(np.ceil(ys.min(0)), y0), np.minimum(np.floor(ys.max(0)), y0 + h - 1)
    ok = np.isfinite(p0).all(1) & np.isfinite(p1).all(1) & np.isfinite(p2).all(1) & (d > np.float32(-999999.0)) & (umax >= umin) & (vmax >= vmin)
    v0x, v0y, v1x, v1y = p2[:, 0] - p0[:, 0], p2[:, 1] - p0[:, 1], p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1]
    dot00, dot01, dot11 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v1x * v1x + v1y * v1y
    det = dot00 * dot11 - dot01 * dot01
    with np.errstate(divide="ignore"):
        inv = np.where(det == 0, 0.0, 1.0 / det)
    bits = d.view(np.uint32)
    ordered = np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
    key = (ordered << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(T, dtype=np.uint64))
    keys = np.zeros(h * w, np.uint64)
    bw, bh = int((umax - umin)[ok].max()) + 1, int((vmax - vmin)[ok].max()) + 1
    for dy in range(bh):
        for dx in range(bw):
            X, Y = umin + dx, vmin + dy
            m = ok & (X <= umax) & (Y <= vmax)
            v2x, v2y = X[m] - p0[m, 0], Y[m] - p0[m, 1]
            dot02, dot12 = v0x[m] * v2x + v0y[m] * v2y, v1x[m] * v2x + v1y[m] * v2y
            bu, bv = (dot11[m] * dot02 - dot01[m] * dot12) * inv[m], (dot00[m] * dot12 - dot01[m] * dot02) * inv[m]
            cover = (bu >= 0) & (bv >= 0) & (bu + bv < 1)
            cell = ((Y[m] - y0) * w + (X[m] - x0)).astype(np.int64)[cover]
            np.maximum.at(keys, cell, key[m][cover])
    win = np.where(keys == 0, -1, (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)).astype(np.int32)
    a = attrs.astype(np.float64)[tri[np.maximum(win, 0)]]                        # [h * w, 3, C]
    image = np.where((win >= 0)[:, None], ((a[:, 0] + a[:, 1] + a[:, 2]) / 3.0).astype(np.float32), np.float32(0))
    return win.reshape(h, w), image.reshape(h, w, -1)


def numpy_colors(pic, v32):
    H, W = pic.shape[:2]
    x = np.round(np.clip(v32[:, 0].astype(np.float64), 0, W - 1)).astype(int)
    y = np.round(np.clip(v32[:, 1].astype(np.float64), 0, H - 1)).astype(int)
    return pic[y, x].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    import face_ab
    from centerpose_amd import config, detector, face, synth
    cap, side = a.capacity, a.window
    rows_, cols_ = np.meshgrid(np.arange(20, 20 + BLOCK), np.arange(20, 20 + BLOCK), indexing="ij")
    face_ind = (rows_ * 256 + cols_).reshape(-1).astype(np.int32)
    tri = face.grid_triangles(face_ind)
    V, T = len(face_ind), len(tri)
    maps, centres = stand_in_maps(cap)
    maps_dev = torch.from_numpy(maps).cuda()
    origin_np = np.floor(centres - side / 2.0).astype(np.int32)
    origin = torch.from_numpy(origin_np).cuda()
    sets = [face_ab.device_frames(1, 480, 640, 300 + 10 * i) for i in range(2)]
    renderer = face.FaceRenderer(face_ind, tri, cap)

    def render_both(frames, result):
        colors = renderer.vertex_colors(frames, result)
        depth = renderer.render(result, size=(side, side), origin=origin)
        return depth, renderer.render(result, size=(side, side), origin=origin, attrs=colors)

    if a.kernels:
        result = face.FaceResult(maps_dev, None, torch.arange(cap, dtype=torch.int32, device="cuda"), None, None)
        for _ in range(a.kernels):
            render_both(sets[0], result)
        torch.cuda.synchronize()
        keys, verts = cap * side * side * 8, cap * T * 3 * 12 + T * 12
        print("floor per render call: keys written and read once %d B + gathered vertices and the triangle table %d B = %.3f MB "
              "(cap %d, window %d, V %d, T %d)" % (2 * keys, verts, (2 * keys + verts) / 1e6, cap, side, V, T))
        return
    al = face.FaceAligner(synth.make_state_dict("prnet", seed=317), face_ab.uv_table(), capacity=cap)
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    vis = float(det.cfg.TEST.VIS_THRESH)

    def path_a(i):
        res = al.align(sets[i & 1], rows=det.run_batch(sets[i & 1], return_device=True), vis_thresh=vis)
        res.pos.copy_(maps_dev)                                                  # the stand-in maps: every path pays this copy
        return res

    def path_b(i):
        res = path_a(i)
        return res, render_both(sets[i & 1], res)

    def path_c(i):
        res = path_a(i)
        pos, slots, pic = res.pos.cpu().numpy(), res.slots.cpu().numpy(), sets[i & 1][0].cpu().numpy()
        out = []
        for s in range(cap):
            if slots[s] < 0:
                continue
            v32 = pos[s].reshape(-1, 3)[face_ind]
            colors = numpy_colors(pic, v32)
            x0, y0 = int(origin_np[s, 0]), int(origin_np[s, 1])
            out.append((numpy_render(v32, tri, x0, y0, side, side, v32[:, 2:3]), numpy_render(v32, tri, x0, y0, side, side, colors)))
        return res, out

    for i in range(2):
        used = path_a(i).slots.cpu().tolist()
        assert all(s >= 0 for s in used), "frame set %d: fewer than %d faces (%s)" % (i, cap, used)
    _, (depth, tex) = path_b(0)
    torch.cuda.synchronize()
    _, host = path_c(0)
    covered = 0
    for s, ((tri_z, img_z), (tri_c, img_c)) in enumerate(host):
        assert np.array_equal(depth.tri[s].cpu().numpy(), tri_z) and np.array_equal(tex.tri[s].cpu().numpy(), tri_c), "slot %d: tri differs" % s
        assert depth.image[s].cpu().numpy().tobytes() == img_z.tobytes() and tex.image[s].cpu().numpy().tobytes() == img_c.tobytes(), s
        covered += int((tri_z >= 0).sum())
    print("(b) equals (c) bit for bit: %d faces, %d of %d window pixels covered per face, V %d, T %d" % (len(host), covered // len(host), side * side, V, T))
    paths = {"a": ("(a) run_batch + align", path_a), "b": ("(b) (a) + vertex_colors + render depth + render colours", path_b),
             "c": ("(c) (a) + maps and frame to the host + vectorised NumPy get_colors and renderer", path_c)}
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
    for rnd in range(a.rounds):
        for k in (keys if rnd % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps[k]):
                paths[k][1](i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    out = {}
    for k in keys:
        v, lo = med[k], min(ms[k])
        spread = 100.0 * (max(ms[k]) - lo) / v
        extra = None if k == "a" else v - med["a"]
        out[k] = {"path": paths[k][0], "ms_per_call_median": round(v, 4), "ms_per_call_min": round(lo, 4), "spread_pct": round(spread, 2),
                  "steps_per_round": steps[k], "minus_a_ms_per_call": None if extra is None else round(extra, 4),
                  "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("480x640 N=1 cap=%-3d window=%-4d %-80s min %9.3f  median %9.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (cap, side, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+9.3f" % extra, steps[k],
                 len(ms[k])), flush=True)
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "capacity": cap, "window": side, "vertices": V, "triangles": T, "paths": out}))


if __name__ == "__main__":
    main()
