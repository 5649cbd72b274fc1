"""What `engine.PlanBuilder` emits, as one line per configuration below: the SHA-256 of the deterministic plan of the synthetic checkpoint
(`plan.plan_blob(engine, deterministic=True)`: the bytes `Engine.save_plan(path, deterministic=True)` writes) and a census of the launches
per kind, per C entry point (":<tile>" = the descriptor's tile code), per "group:" name and per split reduction (the kind of the launch it
finishes + the name's suffix).  Equal lines before and after a change to the builder = the same launches into the same buffers.
usage: python tools/plan_digest.py; CP_BATCH_INVARIANT=1 python tools/plan_digest.py   (read when `ops` is imported: its own process)"""
import collections
import hashlib
import os
import sys
from unittest import mock

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [  # arch, B, H, W, Engine keywords, environment: together they reach every emit path of the builder
    ("dla_34", 1, 128, 128, {}, {}),
    ("dla_34", 4, 512, 512, {}, {}),
    ("dla_34", 1, 128, 128, {"head_conv": 32}, {}),
    ("dla_34", 2, 128, 128, {"decode_k": 100, "flip_test": True}, {}),
    ("dla_34", 1, 128, 128, {}, {"CP_WINOGRAD": "0"}),
    ("dla_34", 1, 128, 128, {}, {"CP_BUFFER_REUSE": "0"}),
    ("dla_34", 4, 512, 512, {}, {"CP_BATCH_INVARIANT": "1"}),
    ("res_50", 8, 512, 512, {}, {}),
    ("res_50", 2, 256, 256, {"decode_k": 100, "dets_only": True}, {}),
    ("resdcn_18", 1, 128, 128, {}, {}),
    ("hrnet", 2, 256, 256, {}, {}),
    ("hrnet", 2, 256, 256, {}, {"CP_GROUP": "0"}),
    ("mobilenetv3", 1, 128, 128, {}, {}),
    ("shufflenetV2", 1, 128, 128, {}, {}),
]


def main():
    from centerpose_amd import engine, ops, plan, synth
    for arch, B, H, W, kw, env in CONFIGS:
        if ("CP_BATCH_INVARIANT" in env) != ops.BATCH_INVARIANT:
            continue
        with mock.patch.dict(os.environ, env):
            eng = engine.Engine(arch, synth.make_state_dict(arch, head_conv=kw.get("head_conv"), H=H, W=W), B, H, W, use_graph=False, **kw)
        n, prev = collections.Counter(), None
        for kind, name, _, launch in eng.emission:
            tile = getattr(launch.desc, "tile", 0)
            tag = "group:" if name.startswith("group:") else prev + name[-7:] if name.endswith((".splitk", ".splitc")) else kind
            n.update({kind, launch.fn + (":%d" % tile if tile else ""), tag})
            prev = kind
        print("%s B=%d %dx%d %s %s sha256=%s launches=%d %s" % (arch, B, H, W, kw or "", env or "", hashlib.sha256(plan.plan_blob(eng, True)).hexdigest(),
                                                           len(eng.emission), " ".join("%s=%d" % kv for kv in sorted(n.items()))), flush=True)


if __name__ == "__main__":
    main()
