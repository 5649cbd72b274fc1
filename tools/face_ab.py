"""Same-process A/B of aligning the faces of run_batch's detections on the device against what a caller had to do without FaceAligner:

  (a)  run_batch(frames, return_device=True)                 detection alone: frames and rows stay on the device
  (b)  (a), then FaceAligner.align(frames, rows=rows)         select + crops (csrc/face_stage.hip), ONE replay of the PRNet plan, restore
  (c)  (a), then what the demo does around its net (demo/face/prnet.py:61-127), kept on the device where it can be: the rows to the
       host, per face a grid_sample crop to 256 x 256, a plain-torch restatement of PRNet on that ONE crop, the map to the host and the
       restore in NumPy, one face after the other as the reference runs them
  (c') (c) with the crops stacked and the plain-torch net run once on the batch

(c) and (c') align exactly the candidates that (b) aligned (its slots and squares), so all paths do the same work; how many that is
per call is printed.  Frames: random bytes with large-scale structure as contiguous BGR [H,W,3] tensors, on the device before any
timing; dla_34 preset as shipped (its own VIS_THRESH); synthetic weights.  Before timing, the landmarks of (c') are compared with (b)'s:
they must agree to 0.05 x size / 255 px (grid_sample is not the crop rule bit for bit; a wrong face or slot would be off by far more).
Every path is warmed, then timed for at least --seconds of work per round; five or more rounds alternate the order of the paths so
drift hits them alike.  Per path: wall ms per call as min / median over rounds and the spread (max - min) / median; this - (a) from
the medians.  There is no pass mark.

  --kernels K   instead of the A/B: K align calls on one frame set and nothing else, for a kernel trace of its own
                (rocprofv3 --kernel-trace --stats -- python tools/face_ab.py --kernels 20)
  --stats CSV   print the kernels of such a trace's kernel_stats CSV, the share of the three-channel tail launches included
usage: python tools/face_ab.py [--sizes 480x640] [--batches 1,4] [--capacity 8] [--rounds 5] [--seconds 0.5]"""
import argparse
import csv
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


def uv_table(seed=5):
    """a stand-in landmark table: the product ships no reference data"""
    return np.random.RandomState(seed).randint(0, 256, (2, 68)).astype(np.int32)


class TorchPRNet:
    """PRNet in plain torch on the device (float32, eval-mode batch norm, eps 1e-3): the restatement a caller would run."""

    def __init__(self, sd, device):
        self.p = {k: v.to(device) for k, v in sd.items()}

    def bn(self, x, q):
        p = self.p
        return F.batch_norm(x, p[q + ".running_mean"], p[q + ".running_var"], p[q + ".weight"], p[q + ".bias"], False, 0.0, 1e-3)

    def same4(self, x, q, stride):
        return F.conv2d(F.pad(x, (1, 2, 1, 2) if stride == 1 else (1, 1, 1, 1)), self.p[q + ".weight"], None, stride)

    def tconv(self, x, q):
        return F.conv_transpose2d(F.pad(x, (2, 1, 2, 1)), self.p[q + ".weight"], None, 1, 3)

    def __call__(self, x):
        p = self.p
        x = F.relu(self.bn(self.same4(x, "input_conv.1", 1), "input_conv.2"))
        for i, stride in enumerate((2, 1, 2, 1, 2, 1, 2, 1, 2, 1), start=1):
            q = "down_conv_%d" % i
            c2, c3 = (3, 6) if stride == 2 else (4, 7)
            h = F.relu(self.bn(F.conv2d(x, p[q + ".main.0.weight"]), q + ".main.1"))
            h = F.relu(self.bn(self.same4(h, "%s.main.%d" % (q, c2), stride), "%s.main.%d" % (q, c2 + 1)))
            h = F.conv2d(h, p["%s.main.%d.weight" % (q, c3)])
            sc = F.conv2d(x, p[q + ".shortcut.weight"], None, stride) if stride == 2 else x
            x = F.relu(self.bn(sc + h, q + ".activate.0"))
        x = F.relu(self.bn(self.tconv(x, "center_conv.1"), "center_conv.2"))
        for i, n in ((5, 2), (4, 2), (3, 2), (2, 1), (1, 1)):
            q = "up_conv_%d.main." % i
            x = F.relu(self.bn(F.conv_transpose2d(x, p[q + "0.weight"], None, 2, 1), q + "1"))
            for j in range(n):
                x = F.relu(self.bn(self.tconv(x, q + str(4 * j + 4)), q + str(4 * j + 5)))
        x = F.relu(self.bn(self.tconv(x, "output_conv.1"), "output_conv.2"))
        x = F.relu(self.bn(self.tconv(x, "output_conv.5"), "output_conv.6"))
        return torch.sigmoid(self.bn(self.tconv(x, "output_conv.9"), "output_conv.10"))


class CallerPath:
    """Paths (c) and (c'): per face a grid_sample crop, the plain-torch net, the map to the host, the restore in NumPy."""

    def __init__(self, net, uv):
        self.net, self.uv = net, uv
        self.lin = torch.arange(256, device="cuda", dtype=torch.float32)

    def crop(self, frame, t):
        H, W = frame.shape[:2]
        x0, y0, size = t
        xs = (x0 + self.lin * (size / 255.0)) * (2.0 / (W - 1)) - 1.0
        ys = (y0 + self.lin * (size / 255.0)) * (2.0 / (H - 1)) - 1.0
        grid = torch.stack([xs.view(1, 256).expand(256, 256), ys.view(256, 1).expand(256, 256)], -1).unsqueeze(0)
        img = frame.permute(2, 0, 1).flip(0).unsqueeze(0).float() / 255.0                  # R, G, B
        return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)

    def restore(self, out, t):
        x0, y0, size = t
        P = out.cpu().numpy().transpose(1, 2, 0) * 256 * 1.1                               # the download the device path does not have
        pos = np.empty_like(P)
        pos[..., 0], pos[..., 1], pos[..., 2] = P[..., 0] * (size / 255.0) + x0, P[..., 1] * (size / 255.0) + y0, P[..., 2] * (size / 255.0)
        return pos, pos[self.uv[1], self.uv[0]]

    def one_by_one(self, frames, used):
        with torch.no_grad():
            return [self.restore(self.net(self.crop(frames[n], t))[0], t) for n, t in used]

    def batched(self, frames, used):
        with torch.no_grad():
            if not used:
                return []
            out = self.net(torch.cat([self.crop(frames[n], t) for n, t in used], 0))
            return [self.restore(o, t) for o, (_, t) in zip(out, used)]


def used_of(res, M):
    """[(frame, (x0, y0, size))] of the slots a FaceResult filled -- read on the host, as a caller reads its rows"""
    s, x = res.slots.cpu().numpy(), res.xform.cpu().numpy()
    return [(int(s[i]) // M, tuple(float(v) for v in x[i])) for i in range(len(s)) if s[i] >= 0]


def ab(det, al, net, H, W, N, a):
    sets = [device_frames(N, H, W, 300 + 10 * i) for i in range(2)]
    caller = CallerPath(net, al.uv_kpt_ind)
    torch.cuda.synchronize()
    vis = float(det.cfg.TEST.VIS_THRESH)
    used = []
    for i in range(2):                                                      # the faces (b) aligns, fixed per frame set, and the cross-check
        rows = det.run_batch(sets[i], return_device=True)
        res = al.align(sets[i], rows=rows, vis_thresh=vis)
        used.append(used_of(res, rows.shape[1]))
        s = res.slots.cpu().numpy()
        want = caller.batched(sets[i], used[i])
        for k, slot in enumerate(np.nonzero(s >= 0)[0]):
            d = float(np.abs(res.landmarks[slot].cpu().numpy() - want[k][1]).max())
            bar = 0.05 * 281.6 * used[i][k][1][2] / 255.0
            assert d <= bar, "device landmarks and the plain-torch path disagree: %.3e px (bar %.3e)" % (d, bar)
    aligned = sum(len(u) for u in used) / 2.0

    def path_a(i):
        return det.run_batch(sets[i & 1], return_device=True)

    def path_b(i):
        return al.align(sets[i & 1], rows=det.run_batch(sets[i & 1], return_device=True), vis_thresh=vis)

    def path_c(i):
        rows = det.run_batch(sets[i & 1], return_device=True)
        rows.cpu()                                                          # the rows to the host: the caller's synchronisation
        return caller.one_by_one(sets[i & 1], used[i & 1])

    def path_d(i):
        rows = det.run_batch(sets[i & 1], return_device=True)
        rows.cpu()
        return caller.batched(sets[i & 1], used[i & 1])

    paths = {"a": ("(a) run_batch", path_a), "b": ("(b) run_batch + align", path_b),
             "c": ("(c) run_batch + torch crops + torch net + NumPy restore, one face at a time", path_c),
             "d": ("(c') the same, crops stacked", path_d)}
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
        print("%4dx%-4d N=%-2d cap=%-3d %4.1f faces/call  %-78s min %8.3f  median %8.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (H, W, N, al.capacity, aligned, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+8.3f" % extra,
                 steps[k], len(ms[k])), flush=True)
    return {"size": [H, W], "N": N, "capacity": al.capacity, "faces_per_call": aligned, "paths": res}


TAIL = ("output_conv.1", "output_conv.5", "output_conv.9")


def print_stats(path):
    """The kernel_stats CSV of a rocprofv3 --kernel-trace --stats run -> its rows, largest first."""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    dur = lambda r: float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
    total = sum(dur(r) for r in rows) or 1.0
    for r in sorted(rows, key=lambda r: -dur(r))[:25]:
        calls = float(r.get("Calls") or 1)
        print("%6.2f %%  calls %6d  avg %10.1f us  %s" % (100 * dur(r) / total, calls, dur(r) / calls / 1e3, r.get("Name", "?")[:110]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x640")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        return print_stats(a.stats)
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    from centerpose_amd import config, detector, face, synth
    sd = synth.make_state_dict("prnet", seed=317)
    al = face.FaceAligner(sd, uv_table(), capacity=a.capacity)
    if a.kernels:
        # the plan's launches one by one on the stream (what the graph replays), so that the trace names every launch; then whole aligns
        frames = device_frames(1, 480, 640, 300)
        boxes = torch.tensor([[[100.0 + 40 * k, 80.0, 220.0 + 40 * k, 230.0, 1.0] for k in range(a.capacity)]], device="cuda")
        prof = al.engine.profile_in_sequence(iters=a.kernels)
        tot = sum(p["ms"] for p in prof)
        tail = sum(p["ms"] for p in prof if p["name"] in TAIL)
        print("plan of %d crops, %d launches in sequence: %.3f ms; the three-channel tail (%s): %.3f ms = %.1f %%"
              % (al.capacity, len(prof), tot, ", ".join(TAIL), tail, 100 * tail / tot))
        for p in sorted(prof, key=lambda p: -p["ms"])[:12]:
            print("  %8.3f ms  %-24s %s" % (p["ms"], p["name"], p["kernel"]))
        for _ in range(a.kernels):
            al.align(frames, boxes=boxes)
        torch.cuda.synchronize()
        return
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    net = TorchPRNet(sd, "cuda")
    out = []
    for s in a.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        for N in (int(n) for n in a.batches.split(",")):
            out.append(ab(det, al, net, H, W, N, a))
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "vis_thresh": float(det.cfg.TEST.VIS_THRESH), "configs": out}))


if __name__ == "__main__":
    main()
