"""Record the PRNet fixtures of tests/golden/ from the reference's own module, on the CPU.

    python tools/make_prnet_golden.py --model <reference checkout>/demo/face/resfcn256.py

This is the only place the reference is imported (by path; the module needs torch alone).  Written:

  tests/golden/prn_keys.json        names and shapes of PRNet(3, 3).state_dict(), in the module's order
  tests/golden/prn_uv_kpt_ind.txt   the reference's landmark table (utils/uv_data/uv_kpt_ind.txt beside the module), byte for byte
  tests/golden/prn_maps.npz         seed        the weights are synth.make_state_dict("prnet", seed) -- the seed is stored, not 53 MB
                                    in_seeds    the inputs are tests/face_ref.make_input(seed, H, W) -- generated, not stored
                                    small       float64 [2,3,64,64]: PRNet(3, 3).eval().double() on the two 64 x 64 inputs, in full
                                    lines       float64 [3,8,256]: of the 256 x 256 input's map, rows 0, 1, 254, 255, then columns
                                                0, 1, 254, 255
                                    grid        float64 [3,32,32]: every 8th pixel of it
                                    landmarks   float64 [3,68]: its 68 landmark cells [:, uv[1], uv[0]]
                                    gap32       the largest difference between the module's own float32 and float64 outputs
                                    (the maps are stored with the low 16 mantissa bits cleared -- 1.5e-11 relative, eight decades
                                    below the 1e-3 bar -- so that the file compresses below the size of the largest fixture)

The module's default init is degenerate (every output in 0.416..0.602 whatever the input), so the tool ASSERTS that each recorded map
has values below 0.2 and above 0.8 and that the landmark cells of any two inputs differ by at least 20 x the 1e-3 parity bar on average:
the synthetic weights must make the map depend on the picture.
"""
import argparse
import importlib.util
import json
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from centerpose_amd import synth  # noqa: E402
import face_ref  # noqa: E402

SEED, SMALL_SEEDS, BIG_SEED, OTHER_BIG_SEED, MIN_DIFF = 317, (11, 12), 21, 22, 0.02
EDGE = (0, 1, 254, 255)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True, help="path of the reference's demo/face/resfcn256.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_resfcn256", a.model)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    keys = [[k, list(v.shape)] for k, v in mod.PRNet(3, 3).state_dict().items()]
    with open(os.path.join(a.out, "prn_keys.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(k) for k in keys) + "\n]\n")
    uv_path = os.path.join(os.path.dirname(os.path.abspath(a.model)), "utils", "uv_data", "uv_kpt_ind.txt")
    shutil.copyfile(uv_path, os.path.join(a.out, "prn_uv_kpt_ind.txt"))
    uv = np.loadtxt(uv_path).astype(np.int32)

    net = mod.PRNet(3, 3).eval()
    net.load_state_dict(synth.make_state_dict("prnet", seed=SEED))

    def run(seed, size):
        x = torch.from_numpy(face_ref.make_input(seed, size, size))[None]
        with torch.no_grad():
            y32 = net.float()(x).double().numpy()[0]
            y64 = net.double()(x.double()).numpy()[0]
        assert y64.min() < 0.2 and y64.max() > 0.8, "input %d at %d: the map spans %.3f..%.3f only" % (seed, size, y64.min(), y64.max())
        return y64, float(np.abs(y32 - y64).max())
    small, big = [run(s, 64) for s in SMALL_SEEDS], run(BIG_SEED, 256)
    other = run(OTHER_BIG_SEED, 256)
    cells = lambda y: y[:, uv[1] * y.shape[1] // 256, uv[0] * y.shape[2] // 256]
    diffs = [float(np.abs(cells(p) - cells(q)).mean()) for p, q in ((small[0][0], small[1][0]), (big[0], other[0]))]
    assert min(diffs) >= MIN_DIFF, "the landmark cells of two inputs differ by %.4g < %.4g on average" % (min(diffs), MIN_DIFF)
    trim = lambda v: (np.ascontiguousarray(v, np.float64).view(np.uint64) & np.uint64(0xFFFFFFFFFFFF0000)).view(np.float64)
    y = big[0]
    gap32 = max(g for _, g in small + [big])
    np.savez_compressed(os.path.join(a.out, "prn_maps.npz"), seed=np.int64(SEED), in_seeds=np.asarray(SMALL_SEEDS + (BIG_SEED,), np.int64),
                        small=trim(np.stack([m for m, _ in small])), lines=trim(np.concatenate([y[:, EDGE, :], y[:, :, EDGE].transpose(0, 2, 1)], 1)),
                        grid=trim(y[:, ::8, ::8]), landmarks=trim(y[:, uv[1], uv[0]]), gap32=np.float64(gap32))
    print("keys %d  gap32 %.3g  landmark-cell differences %s  sizes %s" % (
        len(keys), gap32, ", ".join("%.3f" % d for d in diffs),
        ", ".join("%s %d" % (n, os.path.getsize(os.path.join(a.out, n))) for n in ("prn_keys.json", "prn_uv_kpt_ind.txt", "prn_maps.npz"))))


if __name__ == "__main__":
    main()
