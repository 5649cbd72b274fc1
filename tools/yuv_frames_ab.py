"""Same-process A/B of run_batch fed with device frames as BGR and as NV12 decoder surfaces (480 x 640 pictures, shipped presets):

  (a) BGR device frames     run_batch(list of CUDA uint8 [480,640,3] tensors): the frames read in place
  (b) NV12 surfaces         run_batch(list of CUDA uint8 [720,640] surfaces with a 768-byte pitch, color="nv12"): the planes read in
                            place, converted to BGR where the pre-process loads its taps (csrc/yuv_frames.hip)
  (c) NV12 -> BGR by torch  what a caller had to do without (b): convert every surface to a BGR tensor on the device with torch integer
                            ops (the arithmetic of csrc/yuv_arith.h), then path (a) on the copies

The surfaces and the BGR frames hold the same pictures and are on the device before any timing.  (b) and (c) must return the rows
run_batch returns for the host BGR arrays that the NumPy reference (tests/yuv_ref.py) converts the surfaces to; that is asserted first.
Every path is warmed, then timed for at least --seconds of work per round; rounds alternate the order of the paths so drift hits them
alike.  Per path: wall ms per image as min / median over rounds, and the spread (max - min) / median.
usage: python tools/yuv_frames_ab.py [--configs dla_34:1,dla_34:8,dla_34:16,hrnet:8] [--rounds 5] [--seconds 1.5] [--only abc]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, PITCH = 480, 640, 768


def surfaces(n, seed):
    """n host NV12 surfaces [H*3/2, PITCH] of random bytes (the pitch padding included)."""
    r = np.random.RandomState(seed)
    return [(r.rand(H * 3 // 2, PITCH) * 256).astype(np.uint8) for _ in range(n)]


def reference_bgr(surface):
    import yuv_ref
    return yuv_ref.frame_to_bgr((surface[:H, :W], surface[H:, :W].reshape(H // 2, W // 2, 2)), "nv12")


def torch_nv12_to_bgr(t, coef):
    """One device surface view [H*3/2, W] -> a fresh contiguous uint8 [H,W,3] BGR tensor, by torch integer ops (int32, arithmetic
    shifts): the conversion a caller runs for itself."""
    cy, cvr, cvg, cug, cub, yoff = coef
    y = (t[:H].to(torch.int32) - yoff).clamp_(min=0) * cy
    uv = t[H:].unflatten(1, (W // 2, 2)).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, 0).repeat_interleave(2, 1)
    u, v = uv[..., 0], uv[..., 1]
    half = 1 << 19
    b = (y + cub * u + half) >> 20
    g = (y + cvg * v + cug * u + half) >> 20
    r = (y + cvr * v + half) >> 20
    return torch.stack([b, g, r], -1).clamp_(0, 255).to(torch.uint8)


def ab(arch, N, a):
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg(arch))
    coef = detector.YUV_MATRICES["bt601"]
    host = [surfaces(N, 300 + i) for i in range(2)]
    bgr_host = [[reference_bgr(s) for s in ss] for ss in host]
    nv12 = [[torch.from_numpy(s).cuda()[:, :W] for s in ss] for ss in host]
    bgr = [[torch.from_numpy(im).cuda() for im in imgs] for imgs in bgr_host]
    assert nv12[0][0].stride() == (PITCH, 1)
    torch.cuda.synchronize()

    def path_a(i):
        return det.run_batch(bgr[i & 1])

    def path_b(i):
        return det.run_batch(nv12[i & 1], color="nv12")

    def path_c(i):
        return det.run_batch([torch_nv12_to_bgr(t, coef) for t in nv12[i & 1]])

    paths = {"a": ("(a) BGR device frames", path_a), "b": ("(b) NV12 surfaces", path_b), "c": ("(c) NV12 -> BGR by torch", path_c)}
    keys = [k for k in "abc" if k in a.only]
    # all paths compute the rows of the reference-converted host arrays
    for i in range(2):
        want = det.run_batch(bgr_host[i])
        for k in keys:
            assert paths[k][1](i) == want, "%s: rows differ from run_batch(reference-converted host BGR arrays)" % paths[k][0]
    steps = {}
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
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k] / N)
    res = {}
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    for k in keys:
        v, lo = med[k], min(ms[k])
        spread = 100.0 * (max(ms[k]) - lo) / v
        gain = None if k == "b" or "b" not in med else v - med["b"]
        res[k] = {"path": paths[k][0], "ms_per_image_median": round(v, 4), "ms_per_image_min": round(lo, 4), "spread_pct": round(spread, 2),
                  "steps_per_round": steps[k], "minus_b_ms_per_image": None if gain is None else round(gain, 4),
                  "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-8s N=%-3d %-26s min %7.3f  median %7.3f ms/img  spread %4.1f %%  %s  (%d steps x %d rounds: %s)"
              % (arch, N, paths[k][0], lo, v, spread, "                    " if gain is None else "this - (b) = %+6.3f" % gain, steps[k], len(ms[k]),
                 " ".join("%.3f" % t for t in ms[k])), flush=True)
    return {"arch": arch, "N": N, "scales": list(det.scales), "paths": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="dla_34:1,dla_34:8,dla_34:16,hrnet:8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--only", default="abc")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    out = []
    for c in a.configs.split(","):
        arch, n = c.split(":")
        out.append(ab(arch, int(n), a))
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "image": [H, W], "pitch": PITCH, "configs": out}))


if __name__ == "__main__":
    main()
