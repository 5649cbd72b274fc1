"""Same-process A/B of run_batch fed from host memory and from device memory (uint8 480 x 640 frames, shipped presets):

  (a) host arrays      run_batch(list of numpy arrays): staging copy + one upload of the images, one download of the rows
  (b) device frames    run_batch(list of CUDA uint8 tensors): the frames read in place, no staging, no image upload; one download
  (c) device in/out    run_batch(device tensors, return_device=True) followed by ONE torch.cuda.synchronize(): no download either

The device frames of (b) / (c) are uploaded once, before any timing: the point of the paths is that the producer left them there.
Every path is warmed (plans compiled, graphs captured), then timed for at least --seconds of work per round; rounds alternate the order
of the paths so drift hits them alike.  Per path: wall ms per image as min / median over rounds, and the spread (max - min) / median.
usage: python tools/run_batch_frames_ab.py [--configs dla_34:1,dla_34:8,dla_34:16,hrnet:8] [--rounds 5] [--seconds 1.5] [--only abc]"""
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
    host = [images(N, 300 + i) for i in range(2)]
    dev = [[torch.from_numpy(im).cuda() for im in imgs] for imgs in host]
    torch.cuda.synchronize()

    def path_a(i):
        return det.run_batch(host[i & 1])

    def path_b(i):
        return det.run_batch(dev[i & 1])

    def path_c(i):
        rows = det.run_batch(dev[i & 1], return_device=True)
        torch.cuda.synchronize()
        return rows

    paths = {"a": ("(a) host arrays", path_a), "b": ("(b) device frames", path_b), "c": ("(c) device in/out", path_c)}
    keys = [k for k in "abc" if k in a.only]
    # the three paths compute the same rows
    want = path_a(0)
    if "b" in keys:
        assert path_b(0) == want, "run_batch(device frames) != run_batch(host arrays)"
    if "c" in keys:
        assert np.array_equal(path_c(0).cpu().numpy(), np.array([w[1] for w in want], np.float32)), "return_device rows differ"
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
        gain = None if k == "a" or "a" not in med else med["a"] - v
        res[k] = {"path": paths[k][0], "ms_per_image_median": round(v, 4), "ms_per_image_min": round(lo, 4), "spread_pct": round(spread, 2),
                  "steps_per_round": steps[k], "vs_a_ms_per_image": None if gain is None else round(gain, 4),
                  "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-8s N=%-3d %-18s min %7.3f  median %7.3f ms/img  spread %4.1f %%  %s  (%d steps x %d rounds: %s)"
              % (arch, N, paths[k][0], lo, v, spread, "               " if gain is None else "(a) - this = %+6.3f" % gain, steps[k], len(ms[k]),
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
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "image": [480, 640], "configs": out}))


if __name__ == "__main__":
    main()
