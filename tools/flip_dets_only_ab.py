"""Same-process A/B of detections-only inference under the flip test (the shipped preset: TEST.FLIP_TEST on), inputs = image /
mirrored-twin pairs:

  plans, dla_34 at 512 x 512, 8 and 16 pairs per replay
    (a) dense flip plan      process(x)[1]:    six dense heads for 2N images, two merge launches, decode of the N merged maps
    (b) detections-only      process_dets(x):  hm / hm_hp dense and merged, wh / hps / reg / hp_offset evaluated and merged at the
                                               peaks of the merged heat maps only (cp_head_points_pairs_f32)
  run_batch, N = 8 uint8 480 x 640 images (upload, batched pre-process, one replay, batched post-process, soft-NMS, one download)
    (c) run_batch(images)    (d) run_batch(images, dets_only=True)

Every path is warmed (plans compiled, graphs captured), then timed for at least --seconds of work per round; rounds alternate the
order so drift hits the paths alike.  Per path: the median over rounds of ms per step and per flipped image, with the spread over
rounds ((max - min) / median).  Prints one line per path, the gains with the spread next to them, and a JSON line.
usage: python tools/flip_dets_only_ab.py [--rounds 5] [--seconds 2] [--size 512] [--arch dla_34] [--pairs 8,16] [--only abcd]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--arch", default="dla_34")
    ap.add_argument("--pairs", default="8,16")
    ap.add_argument("--only", default="abcd", help="subset of the paths to run, e.g. 'b' for a profiler run")
    a = ap.parse_args()
    if a.rounds < 5 or a.seconds < 2.0:
        print("note: fewer than five rounds of 2 s: not a number to report", file=sys.stderr)
    from centerpose_amd import config, detector, synth
    cfg = config.get_cfg(a.arch)
    assert cfg.TEST.FLIP_TEST, "the shipped preset runs with the flip test"
    det = detector.MultiPoseDetector(cfg)
    S = a.size

    def pairs(n, seed):
        img = synth.make_images(n, S, S, seed=seed)
        return torch.stack([img, torch.flip(img, [3])], 1).reshape(2 * n, 3, S, S).cuda()

    paths = {}                                       # key -> (name, flipped images per step, step function)
    for n in [int(v) for v in a.pairs.split(",") if v]:
        xs = [pairs(n, 200 + 2 * i) for i in range(2)]
        if "a" in a.only:
            paths["a%d" % n] = ("(a) dense flip plan, %d pairs" % n, n, lambda i, xs=xs: det.process(xs[i & 1]))
        if "b" in a.only:
            paths["b%d" % n] = ("(b) detections-only, %d pairs" % n, n, lambda i, xs=xs: det.process_dets(xs[i & 1]))
    images = [[(np.random.RandomState(300 + 8 * j + i).rand(480, 640, 3) * 255).astype(np.uint8) for i in range(8)] for j in range(2)]
    if "c" in a.only:
        paths["c"] = ("(c) run_batch N=8", 8, lambda i: det.run_batch(images[i & 1]))
    if "d" in a.only:
        paths["d"] = ("(d) run_batch N=8 dets_only", 8, lambda i: det.run_batch(images[i & 1], dets_only=True))
    keys = list(paths)

    steps = {}
    for k in keys:                                   # compile + capture, then size the run to >= --seconds of work
        step = paths[k][2]
        for i in range(3):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(5):
            step(i)
        torch.cuda.synchronize()
        steps[k] = max(10, int(math.ceil(a.seconds / ((time.perf_counter() - t0) / 5))))
    ms = {k: [] for k in keys}
    for r in range(a.rounds):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            step = paths[k][2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps[k]):
                step(i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
    res = {}
    for k in keys:
        name, n, _ = paths[k]
        v = sorted(ms[k])[len(ms[k]) // 2]
        spread = 100.0 * (max(ms[k]) - min(ms[k])) / v
        res[k] = {"path": name, "flipped_images": n, "steps_per_round": steps[k], "ms_per_step": round(v, 4),
                  "ms_per_flipped_img": round(v / n, 4), "spread_pct": round(spread, 2), "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-32s %8.3f ms/step  %7.4f ms/flipped img  spread %.1f %%  (%d steps x %d rounds: %s)"
              % (name, v, v / n, spread, steps[k], a.rounds, " ".join("%.3f" % t for t in ms[k])))
    for dense, sparse in [(k, "b" + k[1:]) for k in keys if k[0] == "a"] + [("c", "d")]:
        if dense in res and sparse in res:
            gain = 100.0 * (1.0 - res[sparse]["ms_per_step"] / res[dense]["ms_per_step"])
            noise = max(res[dense]["spread_pct"], res[sparse]["spread_pct"])
            print("%s -> %s: %+.2f %% time per step (larger spread of the two: %.1f %%)%s"
                  % (res[dense]["path"], res[sparse]["path"], -gain, noise, "  -- INSIDE the spread" if abs(gain) <= noise else ""))
            res[sparse]["gain_pct_vs_dense"] = round(gain, 2)
    print(json.dumps({"arch": a.arch, "size": S, "rounds": a.rounds, "seconds": a.seconds, "paths": res}))


if __name__ == "__main__":
    main()
