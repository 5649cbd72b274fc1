"""Same-process A/B of run_batch fed with the YUV surfaces beyond 8-bit 4:2:0 (480 x 640 pictures, shipped dla_34), in the form of
tools/yuv_frames_ab.py.  Two families of three paths each:

  p010  (a) NV12 surfaces         run_batch(list of CUDA uint8 [720,640] surfaces, 768-byte pitch, color="nv12")
        (b) P010 surfaces         run_batch(list of CUDA uint16 [720,640] surfaces, 1536-byte pitch, color="p010"): read as they are
        (c) P010 -> NV12 by torch what a caller had to do without (b): an 8-bit NV12 copy of every surface by torch integer ops
                                  (sample >> 8), then path (a) on the copies
  i444  (a) BGR device frames     run_batch(list of CUDA uint8 [480,640,3] tensors)
        (b) i444 planes           run_batch(list of (y, u, v) CUDA uint8 [480,640] planes, color="i444", matrix="bt601-full")
        (c) i444 -> BGR by torch  the full-range conversion by torch integer ops (the arithmetic of csrc/yuv_arith.h), then path (a)

The P010 surfaces hold the NV12 samples << 8, so that all three paths of a family compute the same rows; that is asserted first,
against run_batch of the host BGR arrays the NumPy reference (tests/yuv_surface_ref.py) converts the frames to.  Every path is warmed,
then timed for at least --seconds of work per round; rounds alternate the order of the paths so drift hits them alike.  Per path:
wall ms per image as min / median over rounds, and the spread (max - min) / median.  No threshold: (b) is reported against (c) and
against (a), next to the spread.
usage: python tools/yuv_surfaces_ab.py [--configs dla_34:1,dla_34:8,dla_34:16] [--families p010,i444] [--rounds 5] [--seconds 1.5]"""
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

H, W, PITCH = 480, 640, 768          # the pitch in samples: 768 bytes for NV12, 1536 bytes for P010


def torch_p010_to_nv12(t):
    """One device P010 surface view [H*3/2, W] (int16 bit patterns) -> a fresh contiguous uint8 NV12 surface [H*3/2, W]."""
    return ((t.to(torch.int32) & 0xFFFF) >> 8).to(torch.uint8)


def torch_i444_to_bgr(y, u, v, coef):
    """Three device planes [H,W] -> a fresh contiguous uint8 [H,W,3] BGR tensor, by torch integer ops (int32, arithmetic shifts)."""
    cy, cvr, cvg, cug, cub, yoff = coef
    y = (y.to(torch.int32) - yoff).clamp_(min=0) * cy
    u, v = u.to(torch.int32) - 128, v.to(torch.int32) - 128
    half = 1 << 19
    b = (y + cub * u + half) >> 20
    g = (y + cvg * v + cug * u + half) >> 20
    r = (y + cvr * v + half) >> 20
    return torch.stack([b, g, r], -1).clamp_(0, 255).to(torch.uint8)


def family_p010(det, N):
    import yuv_surface_ref as ysr
    r = np.random.RandomState(300)
    host = [[(r.rand(H * 3 // 2, PITCH) * 256).astype(np.uint8) for _ in range(N)] for _ in range(2)]
    bgr_host = [[ysr.frame_to_bgr((s[:H, :W], s[H:, :W].reshape(H // 2, W // 2, 2)), "nv12", "bt601") for s in ss] for ss in host]
    nv12 = [[torch.from_numpy(s).cuda()[:, :W] for s in ss] for ss in host]
    p010 = [[torch.from_numpy((s.astype(np.uint16) << 8).view(np.int16)).cuda()[:, :W] for s in ss] for ss in host]
    assert nv12[0][0].stride() == (PITCH, 1) and p010[0][0].stride() == (PITCH, 1) and p010[0][0].element_size() == 2
    paths = {"a": ("(a) NV12 surfaces", lambda i: det.run_batch(nv12[i & 1], color="nv12")),
             "b": ("(b) P010 surfaces", lambda i: det.run_batch(p010[i & 1], color="p010")),
             "c": ("(c) P010 -> NV12 by torch", lambda i: det.run_batch([torch_p010_to_nv12(t) for t in p010[i & 1]], color="nv12"))}
    return paths, bgr_host


def family_i444(det, N):
    import yuv_surface_ref as ysr
    from centerpose_amd import frames
    coef = frames.SURFACE_MATRICES["bt601-full"]
    r = np.random.RandomState(400)
    host = [[tuple((r.rand(H, W) * 256).astype(np.uint8) for _ in range(3)) for _ in range(N)] for _ in range(2)]
    bgr_host = [[ysr.frame_to_bgr(p, "i444", "bt601-full") for p in ps] for ps in host]
    planes = [[tuple(torch.from_numpy(p).cuda() for p in ps) for ps in pss] for pss in host]
    bgr = [[torch.from_numpy(im).cuda() for im in imgs] for imgs in bgr_host]
    paths = {"a": ("(a) BGR device frames", lambda i: det.run_batch(bgr[i & 1])),
             "b": ("(b) i444 planes, full range", lambda i: det.run_batch(planes[i & 1], color="i444", matrix="bt601-full")),
             "c": ("(c) i444 -> BGR by torch", lambda i: det.run_batch([torch_i444_to_bgr(*p, coef) for p in planes[i & 1]]))}
    return paths, bgr_host


FAMILIES = {"p010": family_p010, "i444": family_i444}


def ab(det, arch, family, N, a):
    paths, bgr_host = FAMILIES[family](det, N)
    torch.cuda.synchronize()
    keys = list("abc")
    for i in range(2):                                        # all paths compute the rows of the reference-converted host arrays
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
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    res = {}
    for k in keys:
        v, lo = med[k], min(ms[k])
        spread = 100.0 * (max(ms[k]) - lo) / v
        gain = None if k == "b" else v - med["b"]
        res[k] = {"path": paths[k][0], "ms_per_image_median": round(v, 4), "ms_per_image_min": round(lo, 4), "spread_pct": round(spread, 2),
                  "steps_per_round": steps[k], "minus_b_ms_per_image": None if gain is None else round(gain, 4),
                  "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-6s %-5s N=%-3d %-28s min %7.3f  median %7.3f ms/img  spread %4.1f %%  %s  (%d steps x %d rounds: %s)"
              % (arch, family, N, paths[k][0], lo, v, spread, "                    " if gain is None else "this - (b) = %+6.3f" % gain, steps[k], len(ms[k]),
                 " ".join("%.3f" % t for t in ms[k])), flush=True)
    return {"arch": arch, "family": family, "N": N, "paths": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="dla_34:1,dla_34:8,dla_34:16")
    ap.add_argument("--families", default="p010,i444")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.5)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    from centerpose_amd import config, detector
    out, dets = [], {}
    for c in a.configs.split(","):
        arch, n = c.split(":")
        if arch not in dets:
            dets[arch] = detector.MultiPoseDetector(config.get_cfg(arch))
        for family in a.families.split(","):
            out.append(ab(dets[arch], arch, family, int(n), a))
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "image": [H, W], "pitch_samples": PITCH, "configs": out}))


if __name__ == "__main__":
    main()
