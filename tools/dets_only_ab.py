"""Same-process A/B of detections-only inference (MultiPoseDetector.process(..., dets_only=True): hm / hm_hp dense, wh / hps / reg /
hp_offset evaluated at the decoded peaks by cp_head_points_f32) against the dense step, dla_34 B = 16 at 512 x 512:

  * process(x)                       vs process(x, dets_only=True)                  (one replay per step)
  * process_stream(depth=2)          vs process_stream(depth=2, dets_only=True)     (two steps in flight, one replay per two)

Rounds alternate the four modes (A B C D, B A D C, ...) so drift hits them alike; per mode the median over rounds of the mean step time.
Prints one line per mode (img/s, ms per step) and a JSON line.
usage: python tools/dets_only_ab.py [--steps 40] [--rounds 5] [--batch 16] [--size 512] [--arch dla_34]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--arch", default="dla_34")
    a = ap.parse_args()
    from centerpose_amd import config, detector, synth
    det = detector.MultiPoseDetector(config.get_cfg(a.arch, TEST__FLIP_TEST=False))
    B, S, n = a.batch, a.size, a.steps
    xs = [synth.make_images(B, S, S, seed=100 + i).cuda() for i in range(2)]

    def one(dets_only):
        def run():
            for i in range(n):
                det.process(xs[i & 1], dets_only=dets_only)
        return run

    def stream(dets_only):
        def run():
            for _ in det.process_stream((xs[i & 1] for i in range(n)), depth=2, dets_only=dets_only):
                pass
        return run

    modes = {"process": one(False), "process dets_only": one(True), "process_stream(depth=2)": stream(False),
             "process_stream(depth=2) dets_only": stream(True)}
    for f in modes.values():             # compile the plans, capture the graphs
        f()
    torch.cuda.synchronize()
    names = list(modes)
    ms = {k: [] for k in names}
    for r in range(a.rounds):
        order = names if r % 2 == 0 else [names[1], names[0], names[3], names[2]]
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            modes[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / n)
    res = {}
    for k in names:
        v = sorted(ms[k])[len(ms[k]) // 2]
        res[k] = {"ms_per_step": round(v, 4), "img_per_s": round(B * 1e3 / v, 1), "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("%-36s %8.1f img/s  %7.3f ms/step   (rounds: %s)" % (k, B * 1e3 / v, v, " ".join("%.3f" % t for t in ms[k])))
    for dense, sparse in ((names[0], names[1]), (names[2], names[3])):
        print("%-36s %+.1f %% img/s" % (sparse + " vs dense", 100.0 * (res[dense]["ms_per_step"] / res[sparse]["ms_per_step"] - 1.0)))
    print(json.dumps({"arch": a.arch, "batch": B, "size": S, "steps": n, "rounds": a.rounds, "modes": res}))


if __name__ == "__main__":
    main()
