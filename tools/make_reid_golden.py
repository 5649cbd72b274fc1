"""Record the re-id fixtures of tests/golden/ from the reference's own module, on the CPU.

    python tools/make_reid_golden.py --model <reference checkout>/demo/tracking/model.py

This is the only place the reference is imported (by path; the module needs torch alone).  Written:

  tests/golden/reid_keys.json     names and shapes of Net().state_dict(), in the module's order
  tests/golden/reid_features.npz  seed      the weights are synth.make_state_dict("reid", seed) -- the seed is stored, not 46 MB of weights
                                  crops     uint8 [8,128,64,3]: eight B, G, R crops with large-scale structure (a random 4 x 2 colour grid
                                            up-sampled bilinearly, +-20 uniform noise, rounded, clipped)
                                  features  float64 [8,512]: Net(reid=True).eval().double() on the crops normalised as the reference's
                                            Extractor does with its defaults ((v - mean[k]) / std[k], no / 255), in float64
                                  gap32     the largest L2 distance between the module's own float32 and float64 features
                                  min_pair  the smallest pairwise L2 distance between the eight float64 features (asserted >= 0.02:
                                            twenty times the 1e-3 parity bar, so a crop in the wrong slot cannot pass)
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centerpose_amd import synth  # noqa: E402
from centerpose_amd.reid import REID_MEAN, REID_STD  # noqa: E402

SEED, CROP_SEED, NCROPS, MIN_PAIR = 317, 20261, 8, 0.02


def make_crops(seed=CROP_SEED, n=NCROPS):
    r = np.random.RandomState(seed)
    grid = torch.from_numpy(r.uniform(0, 255, (n, 3, 4, 2)))
    up = torch.nn.functional.interpolate(grid, size=(128, 64), mode="bilinear", align_corners=False).numpy()
    noisy = up + r.uniform(-20, 20, up.shape)
    return np.clip(np.rint(noisy), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()          # [n,128,64,3]


def normalise(crops, dtype):
    x = torch.from_numpy(crops.astype(np.float64)).permute(0, 3, 1, 2)
    mean = torch.tensor(REID_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(REID_STD, dtype=torch.float64).view(1, 3, 1, 1)
    return ((x - mean) / std).to(dtype)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True, help="path of the reference's demo/tracking/model.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_reid_model", a.model)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    keys = [[k, list(v.shape)] for k, v in mod.Net().state_dict().items()]
    with open(os.path.join(a.out, "reid_keys.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(k) for k in keys) + "\n]\n")

    sd = synth.make_state_dict("reid", seed=SEED)
    net = mod.Net(reid=True).eval()
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("classifier.") for k in missing), (missing, unexpected)
    crops = make_crops()
    with torch.no_grad():
        f32 = net(normalise(crops, torch.float32)).double().numpy()
        f64 = net.double()(normalise(crops, torch.float64)).numpy()
    gap32 = float(np.sqrt(((f32 - f64) ** 2).sum(1)).max())
    d = np.sqrt(((f64[:, None] - f64[None]) ** 2).sum(2))
    min_pair = float(d[~np.eye(NCROPS, dtype=bool)].min())
    assert min_pair >= MIN_PAIR, "the eight features lie too close: smallest pairwise L2 distance %.4g < %.4g" % (min_pair, MIN_PAIR)
    np.savez_compressed(os.path.join(a.out, "reid_features.npz"), seed=np.int64(SEED), crops=crops, features=f64,
                        gap32=np.float64(gap32), min_pair=np.float64(min_pair))
    print("keys %d  gap32 %.3g  min pairwise L2 %.4g  |f| %.6f..%.6f" % (len(keys), gap32, min_pair, np.linalg.norm(f64, axis=1).min(),
                                                                     np.linalg.norm(f64, axis=1).max()))


if __name__ == "__main__":
    main()
