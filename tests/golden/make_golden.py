"""Generates the committed golden vectors by running the REFERENCE implementation
(/root/reference, build container only).  The reference never travels: only the resulting
.npz data files (inputs are regenerated from seeds by tests/cases.py) are committed.

    python tests/golden/make_golden.py [decode] [nets] [dcn] [checks] [spec] [decode_edges]
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference/lib")
warnings.filterwarnings("ignore")

import cases  # noqa: E402


def gen_decode():
    from models.decode import multi_pose_decode, _nms, _topk, _topk_channel
    for name, (gen, kw, K, use_reg, use_off) in cases.DECODE_CASES.items():
        inp = gen(**kw)
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        with torch.no_grad():
            dets = multi_pose_decode(t["hm"], t["wh"], t["hps"], reg=t["reg"] if use_reg else None,
                                     hm_hp=t["hm_hp"], hp_offset=t["hp_offset"] if use_off else None, K=K)
            sc, inds, _, _, _ = _topk(_nms(t["hm"]), K=K + 1)
            hsc, hinds, _, _ = _topk_channel(_nms(t["hm_hp"]), K=K + 1)
        # bit-exact index parity is only defined on tie-free data: check and record
        tie_free = bool((np.diff(sc.numpy().astype(np.float64), axis=-1) < 0).all() and
                        (np.diff(hsc.numpy().astype(np.float64), axis=-1) < 0).all())
        np.savez_compressed(os.path.join(HERE, "decode_%s.npz" % name), dets=dets.numpy(),
                            inds=inds[:, :K].numpy().astype(np.int32),
                            hm_inds=hinds[:, :, :K].numpy().astype(np.int32), tie_free=tie_free)
        print("decode", name, dets.shape, "tie_free", tie_free)


def _ref_decode(inp, K, use_reg=True, use_off=True):
    """The reference's multi_pose_decode with its own top-(K+1) peaks -> (dets, inds, clses, hm_inds, tie_free)."""
    from models.decode import multi_pose_decode, _nms, _topk, _topk_channel
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    with torch.no_grad():
        dets = multi_pose_decode(t["hm"], t["wh"], t["hps"], reg=t["reg"] if use_reg else None,
                                 hm_hp=t["hm_hp"], hp_offset=t["hp_offset"] if use_off else None, K=K)
        sc, inds, clses, _, _ = _topk(_nms(t["hm"]), K=K + 1)
        hsc, hinds, _, _ = _topk_channel(_nms(t["hm_hp"]), K=K + 1)
    tie_free = bool((np.diff(sc.numpy().astype(np.float64), axis=-1) < 0).all() and
                    (np.diff(hsc.numpy().astype(np.float64), axis=-1) < 0).all())
    return (dets.numpy(), inds[:, :K].numpy().astype(np.int32), clses[:, :K].numpy().astype(np.int32),
            hinds[:, :, :K].numpy().astype(np.int32), tie_free)


def distance_ties_are_harmless(cmp):
    """True unless some (image, joint, centre) has its minimum distance at two candidates that differ in position or score --
    the one case in which the reference's `min` over candidates (decode.py:289) could return either of two different answers."""
    tied = cmp["dist"] == cmp["min_dist"][..., None]                                    # [B,J,K,M]
    for key in ("cand_x", "cand_y", "cand_s"):
        v = np.broadcast_to(cmp[key][:, :, None, :], tied.shape)
        first = np.take_along_axis(v, cmp["min_ind"][..., None], axis=3)
        if (tied & (v != first)).any():
            return False
    return True


def gen_decode_edges():
    """decode_edges.npz: the reference's outputs on the decision cases of tests/cases.py (outputs and flags only).
    <case>__specified: the reference's result does not depend on an order torch leaves open (no tie inside the top-(K+1) of any
    plane, no minimum distance shared by different candidates); where it is false the oracle's documented rule is the reference
    (value descending then index ascending, first minimum).  <case>__agrees: the oracle equalled this torch build's output."""
    from oracle import decode_np
    data = {}

    def record(name, inp, K, use_reg=True, use_off=True, clses=False):
        dets, inds, cl, hm_inds, tie_free = _ref_decode(inp, K, use_reg, use_off)
        od, aux = decode_np.multi_pose_decode(inp["hm"], inp["wh"], inp["hps"], inp["reg"] if use_reg else None, inp["hm_hp"],
                                              inp["hp_offset"] if use_off else None, K=K, return_aux=True)
        spec = bool(tie_free and distance_ties_are_harmless(aux["cmp"]))
        agrees = bool(np.array_equal(od, dets) and np.array_equal(aux["inds"], inds) and np.array_equal(aux["hm_inds"], hm_inds))
        data[name + "__dets"], data[name + "__inds"], data[name + "__hm_inds"] = dets, inds, hm_inds
        if clses:
            data[name + "__clses"] = cl
        data[name + "__specified"], data[name + "__agrees"] = np.bool_(spec), np.bool_(agrees)
        print("decode_edges", name, dets.shape, "specified", spec, "oracle agrees", agrees)

    for name, c in cases.decode_assign_edges().items():
        record(name, c["inp"], c["K"], c["use_reg"], c["use_off"])
    for name, (cat, H, W, K, J, seed, seam) in cases.DECODE_MULTICAT_CASES.items():
        record(name, cases.decode_multicat(cat, H, W, J, seed, seam), K, clses=True)
    for name, (seed, H, W, K) in cases.DECODE_SIGNED_CASES.items():
        record(name, cases.decode_signed(seed, H, W), K)
    np.savez_compressed(os.path.join(HERE, "decode_edges.npz"), **data)


def gen_flip():
    """The reference's flip-test merge (multi_pose.py:45-53 with models/utils.py:27-47) on seeded maps."""
    from models.utils import flip_lr, flip_lr_off, flip_tensor
    flip_idx = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]      # multi_pose.py:27
    t = {k: torch.from_numpy(v) for k, v in cases.flip_inputs().items()}
    hm = (t["hm"][0:1] + flip_tensor(t["hm"][1:2])) / 2
    wh = (t["wh"][0:1] + flip_tensor(t["wh"][1:2])) / 2
    hps = (t["hps"][0:1] + flip_lr_off(t["hps"][1:2], flip_idx)) / 2
    hm_hp = (t["hm_hp"][0:1] + flip_lr(t["hm_hp"][1:2], flip_idx)) / 2
    np.savez_compressed(os.path.join(HERE, "flip_merge.npz"), hm=hm.numpy(), wh=wh.numpy(), hps=hps.numpy(),
                        hm_hp=hm_hp.numpy(), reg=t["reg"][0:1].numpy(), hp_offset=t["hp_offset"][0:1].numpy())
    print("flip", tuple(hps.shape))


def gen_checks():
    """What the tests once asked the imported reference for, recorded: multi_pose_decode on two seeded 64x64 batches (K = 50) and
    flip_tensor / flip_lr / flip_lr_off on seeded maps -> reference_checks.npz; the TEST / MODEL settings of the experiment YAMLs
    the presets mirror -> reference_presets.json."""
    import json
    import yaml
    from models import decode as ref_decode
    from models.decode import multi_pose_decode
    from models.utils import flip_lr, flip_lr_off, flip_tensor
    out = {}
    for seed in (0, 1):
        t = {k: torch.from_numpy(v) for k, v in cases.decode_random(100 + seed, B=2, H=64, W=64).items()}
        with torch.no_grad():
            out["decode_seed%d" % seed] = multi_pose_decode(t["hm"], t["wh"], t["hps"], t["reg"], t["hm_hp"], t["hp_offset"], K=50).numpy()
    flip_idx = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]      # multi_pose.py:27
    r = np.random.RandomState(4)
    hp = torch.from_numpy(r.randn(2, 17, 6, 10).astype(np.float32))
    hps = torch.from_numpy(r.randn(2, 34, 6, 10).astype(np.float32))
    out.update(flip_tensor=flip_tensor(hp).numpy(), flip_lr=flip_lr(hp, flip_idx).numpy(), flip_lr_off=flip_lr_off(hps, flip_idx).numpy())
    np.savez_compressed(os.path.join(HERE, "reference_checks.npz"), **out)
    experiments = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(ref_decode.__file__)))), "experiments")
    presets = {}
    for arch, f in (("dla_34", "dla_34_512x512.yaml"), ("res_50", "res_50_512x512.yaml"), ("hrnet", "hrnet_w32_512.yaml"),
                    ("mobilenetv3", "mobilenetv3_512x512.yaml"), ("shufflenetV2", "shufflenetV2_512x512.yaml")):
        y = yaml.safe_load(open(os.path.join(experiments, f)))
        presets[arch] = {"file": "experiments/" + f,
                         "TEST": {k: y["TEST"][k] for k in ("FLIP_TEST", "NMS", "FIX_RES", "TEST_SCALES", "TOPK") if k in y["TEST"]},
                         "MODEL": {k: y["MODEL"][k] for k in ("HEAD_CONV", "INTERMEDIATE_CHANNEL")}}
    with open(os.path.join(HERE, "reference_presets.json"), "w") as fh:
        json.dump(presets, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("checks", sorted(out), "presets", sorted(presets))


if __name__ == "__main__":
    what = sys.argv[1:] or ["decode", "flip", "dcn", "nets"]
    if "decode" in what:
        gen_decode()
    if "decode_edges" in what:
        gen_decode_edges()
    if "flip" in what:
        gen_flip()
    if "checks" in what:
        gen_checks()
    if "dcn" in what or "nets" in what:
        import make_golden_nets
        make_golden_nets.main(what)
    if "spec" in what:
        import make_golden_nets
        make_golden_nets.gen_spec()
