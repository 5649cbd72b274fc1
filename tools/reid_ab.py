"""Same-process A/B of embedding the detections of run_batch on the device against what a caller had to do without ReidExtractor:

  (a)  run_batch(frames, return_device=True)                  detection alone: frames and rows stay on the device
  (b)  run_batch(frames, return_device=True, embed=ex)        the same, then the crops (csrc/reid_crops.hip) and ONE replay of the re-id plan
  (c)  (a), then what DeepSort.update does around its net (demo/tracking/deep_sort.py:24-86), kept on the device: the rows to the host,
       per box a torch slice of the frame, F.interpolate to 128 x 64, normalise, and a plain-torch restatement of the net on that ONE
       crop, one box after the other as the reference runs them
  (c') (c) with the crops stacked and the plain-torch net run once on the batch

(c) and (c') embed exactly the rows that (b) embedded (its slots), so all paths do the same work; how many that is per frame is
printed.  Frames: random bytes with large-scale structure as contiguous BGR [H,W,3] tensors, on the device before any timing; dla_34
preset as shipped (its own VIS_THRESH).  Before timing, the features of (c') are compared with (b)'s: they must agree to 1e-2 in L2
(F.interpolate is not the crop rule bit for bit; a wrong row or slot would be off by far more).  Every path is warmed, then timed for
at least --seconds of work per round; five or more rounds alternate the order of the paths so drift hits them alike.  Per path: wall
ms per call as min / median over rounds and the spread (max - min) / median; this - (a) from the medians.
usage: python tools/reid_ab.py [--sizes 480x640] [--batches 1,4] [--capacity 32] [--rounds 5] [--seconds 0.5]"""
import argparse
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


def device_frames(n, H, W, seed):
    r = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        grid = torch.from_numpy(r.uniform(0, 255, (1, 3, 6, 8)))
        up = F.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
        out.append(torch.from_numpy(np.clip(up + r.uniform(-20, 20, up.shape), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()).cuda())
    return out


class TorchNet:
    """The re-id net in plain torch on the device (float32, eval-mode batch norm): the restatement a caller would run."""

    def __init__(self, sd, device):
        self.p = {k: v.to(device) for k, v in sd.items()}

    def bn(self, x, q):
        p = self.p
        return F.batch_norm(x, p[q + ".running_mean"], p[q + ".running_var"], p[q + ".weight"], p[q + ".bias"], False, 0.0, 1e-5)

    def __call__(self, x):
        p = self.p
        x = F.max_pool2d(F.relu(self.bn(F.conv2d(x, p["conv.0.weight"], p["conv.0.bias"], 1, 1), "conv.1")), 3, 2, 1)
        for li, down in zip(range(1, 5), (False, True, True, True)):
            for b in range(2):
                q, s = "layer%d.%d" % (li, b), 2 if down and b == 0 else 1
                y = F.relu(self.bn(F.conv2d(x, p[q + ".conv1.weight"], None, s, 1), q + ".bn1"))
                y = self.bn(F.conv2d(y, p[q + ".conv2.weight"], None, 1, 1), q + ".bn2")
                if s == 2:
                    x = self.bn(F.conv2d(x, p[q + ".downsample.0.weight"], None, 2, 0), q + ".downsample.1")
                x = F.relu(x + y)
        x = x.mean((2, 3))
        return x / x.norm(p=2, dim=1, keepdim=True)


class CallerPath:
    """Paths (c) and (c'): the per-box crops in torch from the rows on the host, then the plain-torch net."""

    def __init__(self, net, ex):
        from centerpose_amd import reid
        self.net, self.ex = net, ex
        self.mean = torch.tensor(reid.REID_MEAN, device="cuda").view(1, 3, 1, 1)
        self.std = torch.tensor(reid.REID_STD, device="cuda").view(1, 3, 1, 1)

    def crops(self, frames, rows, slots):
        rows_h, M = rows.cpu().numpy(), rows.shape[1]                       # the synchronisation the device path does not have
        out = []
        for idx in slots:
            n, m = divmod(int(idx), M)
            H, W = frames[n].shape[:2]
            x1, y1, x2, y2 = (int(v) for v in rows_h[n, m, :4])
            w, h = x2 - x1, y2 - y1
            x1, y1 = max(x1, 0), max(y1, 0)
            x2, y2 = min(x1 + w, W - 1), min(y1 + h, H - 1)
            c = frames[n][y1:y2, x1:x2].permute(2, 0, 1).unsqueeze(0).float()
            out.append((F.interpolate(c, size=(128, 64), mode="bilinear", align_corners=False) - self.mean) / self.std)
        return out

    def one_by_one(self, frames, rows, slots):
        with torch.no_grad():
            return [self.net(c) for c in self.crops(frames, rows, slots)]

    def batched(self, frames, rows, slots):
        with torch.no_grad():
            c = self.crops(frames, rows, slots)
            return self.net(torch.cat(c, 0)) if c else torch.zeros((0, 512), device="cuda")


def ab(det, ex, net, H, W, N, a):
    sets = [device_frames(N, H, W, 300 + 10 * i) for i in range(2)]
    caller = CallerPath(net, ex)
    torch.cuda.synchronize()
    used = []
    for i in range(2):                                                      # the rows (b) embeds, fixed per frame set, and the cross-check
        rows, res = det.run_batch(sets[i], return_device=True, embed=ex)
        s = res.slots.cpu().numpy()
        used.append([int(v) for v in s[s >= 0]])
        if used[i]:
            got = res.features[torch.from_numpy(s >= 0).cuda()]
            want = caller.batched(sets[i], rows, used[i])
            d = float((got - want).norm(dim=1).max())
            assert d <= 1e-2, "device embeddings and the plain-torch path disagree: L2 %.3e" % d
    embedded = sum(len(u) for u in used) / 2.0

    def path_a(i):
        return det.run_batch(sets[i & 1], return_device=True)

    def path_b(i):
        return det.run_batch(sets[i & 1], return_device=True, embed=ex)

    def path_c(i):
        return caller.one_by_one(sets[i & 1], det.run_batch(sets[i & 1], return_device=True), used[i & 1])

    def path_d(i):
        return caller.batched(sets[i & 1], det.run_batch(sets[i & 1], return_device=True), used[i & 1])

    paths = {"a": ("(a) run_batch", path_a), "b": ("(b) run_batch(embed=)", path_b),
             "c": ("(c) run_batch + torch crops + torch net, one box at a time", path_c),
             "d": ("(c') run_batch + torch crops + torch net, batched", path_d)}
    keys, steps = list("abcd"), {}
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
        print("%4dx%-4d N=%-2d cap=%-3d %4.1f crops/call  %-60s min %8.3f  median %8.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (H, W, N, ex.capacity, embedded, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+8.3f" % extra,
                 steps[k], len(ms[k])), flush=True)
    return {"size": [H, W], "N": N, "capacity": ex.capacity, "crops_per_call": embedded, "paths": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x640")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--capacity", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    from centerpose_amd import config, detector, reid, synth
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    sd = synth.make_state_dict("reid", seed=317)
    ex = reid.ReidExtractor(sd, capacity=a.capacity)
    net = TorchNet(sd, "cuda")
    out = []
    for s in a.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        for N in (int(n) for n in a.batches.split(",")):
            out.append(ab(det, ex, net, H, W, N, a))
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "vis_thresh": float(det.cfg.TEST.VIS_THRESH), "configs": out}))


if __name__ == "__main__":
    main()
