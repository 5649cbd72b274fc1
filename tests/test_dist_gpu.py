"""GPU: the N>1 path of bench.py as the driver launches it -- `python bench.py --gpus N` with NO launcher around it must
spawn one rank per GPU itself (torch.distributed.run, 127.0.0.1 rendezvous), shard the global batch, gather the decoded
poses and print one JSON line whose `ranks` is the world size the process group saw.

* >= 2 visible devices: world_size 2 over nccl (RCCL), one GPU per rank.
* 1 visible device (the gpurun box): the same control flow with both ranks on GPU 0 over gloo (CP_DIST_BACKEND=gloo):
  RCCL cannot place two ranks on one device, the launcher / sharding / gather / timing code is identical.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(env_extra, gpus=2, batch=2, extra=()):
    env = dict(os.environ, **env_extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "3", "--warmup", "2", "--batch", str(batch),
                        "--no-cpu-baseline", "--no-profile", "--gather-check"] + list(extra), capture_output=True, text=True, timeout=1500,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    multi = torch.cuda.device_count() >= 2
    line = _bench({} if multi else {"CP_DIST_BACKEND": "gloo"})
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and line["backend"] == ("nccl" if multi else "gloo")
    assert line["config"]["global_batch"] == 4 and line["scaling"] == "weak" and line["value"] > 0
    assert line["steps"] == 3 and abs(line["value"] - 4 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-3
    # round 3: what the first real multi-GPU run will be read by -- per-rank step times, the exposed wait for the side-stream
    # gather, how the graph was captured, and the cross-rank checksum of the gathered detections
    assert 0 < line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"] == line["ms_per_step"]
    assert line["graph_capture"] == "2-stream" and line["gather"]["check"].startswith("ok: 2 ranks")
    assert line["gather"]["exposed_wait_ms_per_step"]["max_over_ranks"] >= 0.0


def test_bench_eight_rank_dress_rehearsal():
    """the first real 8-GPU run will be the driver's, unattended -- so the whole N = 8 control flow runs HERE first, on
    whatever the box has: `python bench.py --gpus 8 --batch 2 --steps 3 --gather-check` (BASELINE configs[3]'s world size; batch 2
    per rank so that 8 x 2 plan instances share one device).  With 8 visible devices it is the real thing over RCCL; with fewer the
    ranks share the devices round-robin over gloo (RCCL cannot place two ranks on one device): self-launch under
    torch.distributed.run, rendezvous on 127.0.0.1, per-rank plan compilation and schedule measurement under contention, sharding
    of the global batch of 16, the side-stream gather, max-over-ranks timing, `ranks: 8`, the cross-rank checksum."""
    full = torch.cuda.device_count() >= 8
    line = _bench({} if full else {"CP_DIST_BACKEND": "gloo"}, gpus=8)
    assert line["n_gpus"] == 8 and line["ranks"] == 8 and line["backend"] == ("nccl" if full else "gloo")
    assert line["config"]["global_batch"] == 16 and line["config"]["parallelism"] == "dp8" and line["scaling"] == "weak"
    assert line["value"] > 0 and abs(line["value"] - 16 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-3
    assert 0 < line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"] == line["ms_per_step"]
    assert line["graph_capture"] == "2-stream" and line["gather"]["check"].startswith("ok: 8 ranks")
    assert "MultiPoseDetector.process_stream" in line["config"]["entry_point"] and line["config"]["steps_in_flight"] == 2


def test_bench_two_ranks_hrnet_configs4_shape():
    """BASELINE configs[4]'s per-GPU shape through the N > 1 path: `bench.py --arch hrnet --batch 8 --gpus 2` (HRNet-W32, 8 images per
    rank, two ranks; over RCCL with two devices, else both ranks on device 0 over gloo)."""
    multi = torch.cuda.device_count() >= 2
    line = _bench({} if multi else {"CP_DIST_BACKEND": "gloo"}, gpus=2, batch=8, extra=("--arch", "hrnet"))
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and "HRNet-W32" in line["metric"] and "hrnet 512x512 batch=8" in line["config"]["workload"]
    assert line["config"]["global_batch"] == 16 and line["value"] > 0 and line["gather"]["check"].startswith("ok: 2 ranks")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two MI355X for an RCCL world of 2")
def test_gather_dets_over_rccl_matches_single_process(tmp_path):
    """world_size 2 over nccl: every rank's gathered detections equal the single-process decode of the global batch."""
    code = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import cases
from centerpose_amd import dist as cpd
from centerpose_amd.decode import multi_pose_decode
rank, world, local = cpd.init_from_env("nccl")
torch.cuda.set_device(local)
inp = {k: torch.from_numpy(v).cuda() for k, v in cases.decode_random(5, B=5).items()}
full = multi_pose_decode(inp["hm"], inp["wh"], inp["hps"], inp["reg"], inp["hm_hp"], inp["hp_offset"], K=100)
lo, hi = cpd.shard_range(5, rank, world)
mine = multi_pose_decode(*(inp[k][lo:hi] for k in ("hm", "wh", "hps", "reg", "hm_hp", "hp_offset")), K=100)
g = cpd.DetsGatherer(global_batch=5)
g.submit(mine)
got = g.collect()
torch.cuda.synchronize()
assert torch.equal(got, full), "rank %d" % rank
dist.barrier(); dist.destroy_process_group()
"""
    script = tmp_path / "rccl_gather.py"
    script.write_text(code)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29517", str(script), ROOT], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_rccl_world_of_one_gatherer_on_side_stream(tmp_path):
    """RCCL on the hardware a one-GPU lease has: a process group of ONE rank over nccl, `DetsGatherer(force=True)`:
    the all_gather_into_tensor really runs as an RCCL kernel on the side stream while the next hipGraph replay of the engine runs
    on the compute stream.  Proves communicator creation, the collective launch, the event ordering against graph replays and the
    record_stream lifetimes -- everything of SURVEY 8e except the xGMI wire.  Bit-equal dets, sane exposed wait, clean shutdown."""
    code = r"""
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from centerpose_amd import dist as cpd, engine, synth
rank, world, local = cpd.init_from_env("nccl", force=True)
assert (rank, world) == (0, 1) and dist.get_backend() == "nccl" and dist.get_world_size() == 1
torch.cuda.set_device(0)
B = 2
eng = engine.Engine("dla_34", synth.make_state_dict("dla_34"), B, 128, 128, device="cuda", use_graph=True, decode_k=100)
imgs = [synth.make_images(B, 128, 128, seed=40 + i).cuda() for i in range(6)]
want = []
for x in imgs:                                   # reference pass: no gatherer at all
    eng.input.copy_(x)
    want.append(eng.process(eng.input)[1].clone())
torch.cuda.synchronize()
gat = cpd.DetsGatherer(global_batch=B, time_waits=True, force=True)
assert gat.active and gat.side is not None and gat.time_waits
got = []
for x in imgs:                                   # pipelined: gather of step i runs beside the replay of step i + 1
    eng.input.copy_(x)
    _, dets = eng.process(eng.input)
    if gat.pending:
        got.append(gat.collect())
    gat.submit(dets.clone())
got.append(gat.collect())
torch.cuda.synchronize()
assert len(got) == len(want)
for i, (g, w) in enumerate(zip(got, want)):
    assert g.shape == (B, 100, 56) and torch.equal(g, w), "step %d: gathered dets differ" % i
total, worst = gat.exposed_wait_ms()
assert 0.0 <= worst <= total < 1000.0, (total, worst)
ok, csum, msg = cpd.check_gathered(cpd.gather_dets(want[-1], B, force=True), want[-1], B)
assert ok, msg
t0 = time.time()
dist.barrier(); dist.destroy_process_group()
print("RCCL1_OK exposed_wait_ms total %.3f worst %.3f; %s; shutdown %.2f s" % (total, worst, msg, time.time() - t0))
"""
    script = tmp_path / "rccl_world1.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "RCCL1_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout.strip().splitlines()[-1])


def test_bench_force_gather_runs_rccl_on_one_gpu():
    """`bench.py --gpus 1 --force-gather`: the N = 1 line with `backend: "nccl"`, `ranks: 1` and the gather diagnostics of the
    N > 1 line (exposed wait of the side-stream collective, cross-rank checksum)."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CP_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-gather", "--steps", "4", "--warmup", "2",
                        "--batch", "2", "--no-cpu-baseline", "--no-profile", "--gather-check"], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["n_gpus"] == 1 and line["ranks"] == 1 and line["backend"] == "nccl" and line["value"] > 0
    g = line["gather"]
    assert g["check"].startswith("ok: 1 ranks") and "HIP events" in g["timed_with"]
    assert 0.0 <= g["exposed_wait_ms_per_step"]["max_over_ranks"] < line["ms_per_step"]


def test_bench_single_gpu_line_contract():
    """`python bench.py` as the driver runs it at N = 1 (short): ONE JSON line with the contract's keys, the metric / workload of
    BASELINE.json configs[2], dtype f32, a `roofline` object whose dominant-kernel time fits inside the step and whose fraction is
    achieved / peak, and -- with --no-cpu-baseline absent -- a `cpu_baseline` that says which thread count it used."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--steps", "5", "--warmup", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["warmup"] == 2 and line["dtype"] == "f32" and line["vs_baseline"] is None
    assert "DLA-34 512" in line["metric"] and "dla_34 512x512 batch=16" in line["config"]["workload"] and line["scaling"] == "weak"
    assert abs(line["value"] - 16 * 5 / (line["ms_per_step"] * 5e-3)) / line["value"] < 1e-3
    roof = line["roofline"]
    assert roof["bound"] == "mfma" and roof["peak"] == 157.3 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    dom_ms = sum(v["ms_per_step"] for k, v in roof["kernels"].items() if k.startswith(roof["kernel"]))
    assert 0 < dom_ms < line["ms_per_step"] and 0.3 < roof["frac"] < 1.0
    assert line["graph_capture"] == "2-stream" and line["gather"] is None and line["ranks"] == 1
    # configs[1] and the per-GPU shape of configs[4] ride behind the timed region as `other_configs`
    for k in ("res_50_b8", "hrnet_b8"):
        oc = line["other_configs"][k]
        assert "error" not in oc, oc
        assert oc["images_per_sec"] > 0 and oc["graph_capture"] == "2-stream" and 0.2 < oc["all_mfma_executed_frac"] < 1.0
        assert 0.1 < oc["min_bound_frac"]["of_in_sequence"] <= 1.0
    # round 5: what a reader had to recompute -- the min-bound fraction, per-template traffic ratios from
    # the committed PMC passes, a sustained figure over >= 1000 replays -- and (#1) the opt-in split-bf16 evidence run
    mb = roof["min_bound_frac"]
    assert 0.3 < mb["of_in_sequence"] <= 1.0 and 0.3 < mb["of_wall_step"] <= 1.05 and mb["bound_ms_per_step"] < line["ms_per_step"]
    assert all(0.0 < t["min_bound_frac"] <= 1.05 for t in roof["templates"].values())
    assert any("traffic_ratio" in t for t in roof["templates"].values())
    # round 5: two steps in flight by default (engine.EnginePipeline's arrangement); the one-replay-after-the-other figure of rounds
    # 1-4 rides along and cannot be faster than the pipelined one by more than noise
    assert line["config"]["steps_in_flight"] == 2 and "instances of the compiled plan" in line["config"]["pipeline"]
    assert 0.7 * line["value"] < line["one_step_in_flight"]["images_per_sec"] < 1.03 * line["value"]
    # round 6: the headline goes through the product entry point, says how many images one replay holds and
    # what a batch's latency is, and carries the one-step-per-replay figure INSIDE `config` (the part of the line the driver keeps)
    cfgl = line["config"]
    assert "MultiPoseDetector.process_stream" in cfgl["entry_point"] and cfgl["images_per_replay"] == 32
    assert abs(cfgl["batch_latency_ms"] - 2 * line["ms_per_step"]) < 0.01
    assert cfgl["one_step_in_flight"] == line["one_step_in_flight"] and "MultiPoseDetector.process(" in cfgl["one_step_in_flight"]["entry_point"]
    assert roof["one_step_in_flight_images_per_sec"] == line["one_step_in_flight"]["images_per_sec"]
    sus = line["sustained"]
    assert sus["steps"] >= 1000 and 0.8 * line["value"] < sus["images_per_sec"] < 1.2 * line["value"]
    # the kernels this line timed, for tests/test_engine_hip.py::test_timed_configuration_parity of the SAME pytest session (it runs
    # later: "test_dist_gpu" < "test_engine_hip") -- tested kernels == timed kernels as a hard assertion again
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "timed_kernels_dla_34.json"), "w") as f:
            json.dump({"kernels": sorted(roof["kernels"]), "from": "bench.py --gpus 1 --full --steps 5 --warmup 2 --no-cpu-baseline"}, f, indent=1)
    except OSError as e:
        print("could not write the timed-kernel list:", e)
    sb = line["other_configs"]["res_50_b8_split_bf16"]
    assert "error" not in sb, sb
    assert "igemm_bf16x3_kernel" in sb["templates"] and "CP_SPLIT_BF16=1" in sb["mode"] and sb["images_per_sec"] > 0
