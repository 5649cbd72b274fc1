"""Same-process A/B of the ways from N images in host memory to N result lists in host memory (uint8 480 x 640 images, shipped presets):

  (a) run loop      run(image) per image -- the only entry point before run_batch, the baseline
  (b) manual        torch.cat of N pre_process calls, ONE process, a loop of post_process / merge_outputs (one scale), or that per scale
  (c) run_batch     run_batch(images)
  (p) process only  process alone on the same device batch (per scale): what (c) cannot go below; (x) - (p) is printed as the
                    "host + pre/post" cost per image of path x

Every path is warmed (plans compiled, graphs captured), then timed for at least --seconds of work per round; rounds alternate the order
of the paths so drift hits them alike.  Per path: the median over rounds of wall ms per image, with the spread over rounds.
--nms: instead, the merge stage alone -- the device soft-NMS launch (R = 100 and 200 rows, 1 and 8 images, hipEvent time) next to the
host function's time for the same rows.  --steps K: K steps per path, one round, no sizing (for a profiler run).
usage: python tools/run_batch_ab.py [--configs dla_34:1,dla_34:8,dla_34:16,hrnet:8] [--rounds 3] [--seconds 2] [--only abcp] [--nms]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def images(n, seed, h=480, w=640):
    r = np.random.RandomState(seed)
    return [(r.rand(h, w, 3) * 255).astype(np.uint8) for _ in range(n)]


def ab(arch, N, a):
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg(arch))
    sets = [images(N, 300 + i) for i in range(2)]
    scales = det.scales
    dev = [[torch.cat([det.pre_process(im, s)[0] for im in imgs], 0) for s in scales] for imgs in sets]       # for (p)

    def path_a(imgs, i):
        return [det.run(im)["results"] for im in imgs]

    def path_b(imgs, i):
        per_image = [[] for _ in imgs]
        for s in scales:
            pre = [det.pre_process(im, s) for im in imgs]
            _, dets = det.process(torch.cat([x for x, _ in pre], 0))
            for n, (_, meta) in enumerate(pre):
                per_image[n].append(det.post_process(dets[n:n + 1], meta, s))
        return [{1: det.merge_outputs(p)} for p in per_image]

    def path_c(imgs, i):
        return det.run_batch(imgs)

    def path_p(imgs, i):
        for x in dev[i & 1]:
            det.process(x)
        torch.cuda.synchronize()

    paths = {"a": ("(a) run loop", path_a), "b": ("(b) manual", path_b), "c": ("(c) run_batch", path_c), "p": ("(p) process only", path_p)}
    keys = [k for k in "abcp" if k in a.only]
    steps = {}
    for k in keys:
        for i in range(2):
            paths[k][1](sets[i & 1], i)
        torch.cuda.synchronize()
        if a.steps:
            steps[k] = a.steps
            continue
        t0 = time.perf_counter()
        for i in range(3):
            paths[k][1](sets[i & 1], i)
        torch.cuda.synchronize()
        steps[k] = max(3, int(math.ceil(a.seconds / ((time.perf_counter() - t0) / 3))))
    ms = {k: [] for k in keys}
    for r in range(1 if a.steps else a.rounds):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps[k]):
                paths[k][1](sets[i & 1], i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k] / N)
    res = {}
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    for k in keys:
        v = med[k]
        spread = 100.0 * (max(ms[k]) - min(ms[k])) / v
        over = v - med["p"] if "p" in med and k != "p" else None
        res[k] = {"path": paths[k][0], "ms_per_image": round(v, 4), "spread_pct": round(spread, 2), "steps_per_round": steps[k],
                  "host_pre_post_ms_per_image": None if over is None else round(over, 4), "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-8s N=%-3d %-18s %8.3f ms/img  spread %4.1f %%  %s  (%d steps x %d rounds: %s)"
              % (arch, N, paths[k][0], v, spread, "               " if over is None else "- (p) = %6.3f" % over, steps[k], len(ms[k]),
                 " ".join("%.3f" % t for t in ms[k])), flush=True)
    return {"arch": arch, "N": N, "paths": res}


def nms_compare():
    from centerpose_amd import detector
    for R in (100, 200):
        for N in (1, 8):
            r = np.random.RandomState(R + N)
            b = r.rand(N, R, 56).astype(np.float32)
            b[:, :, 0:2] *= 500
            b[:, :, 2:4] = b[:, :, 0:2] + (r.rand(N, R, 2) * 60 + 20).astype(np.float32)
            b[:, :, 4] = (0.97 * 0.98 ** (r.permutation(R) * (400.0 / R))).astype(np.float32)
            t0 = time.perf_counter()
            reps = 50
            for _ in range(reps):
                for n in range(N):
                    detector.soft_nms_39(b[n].copy(), Nt=0.5, method=2)
            host_us = (time.perf_counter() - t0) * 1e6 / reps
            d = torch.from_numpy(b).cuda()
            for _ in range(3):
                detector.post_merge_batch([d], nms=True, Nt=0.5, method=2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                detector.post_merge_batch([d], nms=True, Nt=0.5, method=2)
            e1.record()
            torch.cuda.synchronize()
            print("soft-NMS R=%d rows x N=%d images: host cp_soft_nms_39 %.1f us for the N images (%.1f us per image), device "
                  "cp_post_merge_batch_f32 %.1f us per launch of N images (stream time, launches back to back)"
                  % (R, N, host_us, host_us / N, e0.elapsed_time(e1) * 1e3 / reps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="dla_34:1,dla_34:8,dla_34:16,hrnet:8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--only", default="abcp")
    ap.add_argument("--nms", action="store_true")
    a = ap.parse_args()
    if a.nms:
        nms_compare()
        return
    out = []
    for c in a.configs.split(","):
        arch, n = c.split(":")
        out.append(ab(arch, int(n), a))
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "image": [480, 640], "configs": out}))


if __name__ == "__main__":
    main()
