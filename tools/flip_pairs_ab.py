"""Same-process A/B of the flip test (the shipped preset: TEST.FLIP_TEST on), dla_34 at 512 x 512, inputs = image / mirrored-twin pairs:

  (a) two-stage, B = 2     process(x, return_time=True): forward replay, sync, per-pair merge launches + decode, sync (run()'s path)
  (b) one replay, B = 2    process(x): merge and decode inside the plan's two-stream hipGraph
  (c) one replay, 8 pairs  process(x) at B = 16
  (d) one replay, 16 pairs process(x) at B = 32

Every path is warmed (plans compiled, graphs captured), then timed for at least --seconds of work per round; rounds alternate the
order (a b c d, d c b a, ...) so drift hits the paths alike.  Per path: the median over rounds of ms per step and flipped images/s
(pairs per second), with the spread over rounds.  Prints one line per path and a JSON line.
usage: python tools/flip_pairs_ab.py [--rounds 5] [--seconds 2] [--size 512] [--arch dla_34] [--only c]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--arch", default="dla_34")
    ap.add_argument("--only", default="abcd", help="subset of the paths to run, e.g. 'c' for a profiler run")
    a = ap.parse_args()
    from centerpose_amd import config, detector, synth
    cfg = config.get_cfg(a.arch)
    assert cfg.TEST.FLIP_TEST, "the shipped preset runs with the flip test"
    det = detector.MultiPoseDetector(cfg)
    S = a.size

    def pairs(n, seed):
        img = synth.make_images(n, S, S, seed=seed)
        return torch.stack([img, torch.flip(img, [3])], 1).reshape(2 * n, 3, S, S).cuda()

    paths = {"a": ("(a) two-stage B=2", 1, True), "b": ("(b) one replay B=2", 1, False),
             "c": ("(c) one replay 8 pairs", 8, False), "d": ("(d) one replay 16 pairs", 16, False)}
    keys = [k for k in "abcd" if k in a.only]
    xs = {k: [pairs(paths[k][1], 200 + 2 * i) for i in range(2)] for k in keys}

    def step(k, i):
        _, npairs, timed = paths[k]
        if timed:
            det.process(xs[k][i & 1], return_time=True)
        else:
            det.process(xs[k][i & 1])

    steps = {}
    for k in keys:                                   # compile + capture, then size the run to >= --seconds of work
        for i in range(3):
            step(k, i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(5):
            step(k, i)
        torch.cuda.synchronize()
        steps[k] = max(10, int(math.ceil(a.seconds / ((time.perf_counter() - t0) / 5))))
    ms = {k: [] for k in keys}
    for r in range(a.rounds):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps[k]):
                step(k, i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
    res = {}
    for k in keys:
        name, npairs, _ = paths[k]
        v = sorted(ms[k])[len(ms[k]) // 2]
        spread = 100.0 * (max(ms[k]) - min(ms[k])) / v
        res[k] = {"path": name, "pairs": npairs, "steps_per_round": steps[k], "ms_per_step": round(v, 4),
                  "flipped_img_per_s": round(npairs * 1e3 / v, 1), "ms_per_flipped_img": round(v / npairs, 4),
                  "spread_pct": round(spread, 2), "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-26s %8.1f flipped img/s  %8.3f ms/step  %7.3f ms/img  spread %.1f %%  (%d steps x %d rounds: %s)"
              % (name, npairs * 1e3 / v, v, v / npairs, spread, steps[k], a.rounds, " ".join("%.3f" % t for t in ms[k])))
    print(json.dumps({"arch": a.arch, "size": S, "rounds": a.rounds, "seconds": a.seconds, "paths": res}))


if __name__ == "__main__":
    main()
