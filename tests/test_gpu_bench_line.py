"""bench.py end to end on the visible GPUs (the driver's command line at N = torch.cuda.device_count()): one JSON line with the
contract keys; with --full also the roofline / cpu_baseline objects, every BASELINE config under other_configs, and per-rank device
evidence; --dump-outputs writes the last timed step's scores."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_end_to_end_on_the_visible_gpus():
    import torch
    n = torch.cuda.device_count()
    assert n >= 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "2", "--other-steps", "3",
           "--cpu-clouds", "1", "--no-other-precisions", "--full"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "windows", "ranks"):
        assert key in line, key
    assert line["n_gpus"] == n and line["steps"] == 3 and line["value"] > 0
    assert line["ranks"]["world"] == n and line["ranks"]["distinct_devices"] == n and len(line["ranks"]["devices"]) == n
    assert len({(d["uuid"], d["pci"]) for d in line["ranks"]["devices"]}) == n
    assert len(line["windows"]["clouds_per_s"]) == 3
    assert line["roofline"]["frac"] > 0
    if n == 1:
        assert line["parity_checked"]["ok"] and line["parity_checked"]["node_ids_bit_exact_all_clouds"]["ok"]
        assert line["cpu_baseline"]["value"] > 0
        oc = line["other_configs"]
        for key in ("configs[1] train bf16", "configs[1] train h3", "configs[2] segmenter", "configs[3] autoencoder"):
            assert key in oc and "error" not in oc[key], (key, oc.get(key))
            assert oc[key]["clouds_per_s"] > 0 and oc[key]["parity_checked"]["ok"], (key, oc[key]["parity_checked"])
        assert oc["configs[1] train bf16"]["allreduce"]["backend"] == "nccl"
        train_keys = ["configs[1] train bf16", "configs[1] train h3"]
    else:
        # the driver's multi-GPU command: the forward line above AND BASELINE configs[4] (data-parallel training, RCCL all-reduce)
        oc = line["other_configs"]
        train_keys = ["configs[4] train bf16", "configs[4] train h3"]
    for key in train_keys:
        e = oc[key]
        assert e["n_gpus"] == n and e["global_batch"] == n * e["batch_per_gpu"] and e["clouds_per_s"] > 0
        assert e["allreduce"]["rccl_world_size"] == n and e["allreduce"]["bytes_per_step"] > 0 and e["allreduce"]["exposed_us_per_step"] >= 0
        assert 0 < e["per_rank_ms_per_step"]["min"] <= e["per_rank_ms_per_step"]["max"] <= e["ms_per_step"] * 1.5
        assert e["parity_checked"]["ok"]


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times the headline only and prints its keys; --dump-outputs writes the scores of the last timed step:
    6 steps round-robin over 4 graphs end on graph 1, whose batch (seed 100 + 1000) the eager forward here recomputes bit for bit."""
    import numpy as np
    import torch
    import bench
    from models import networks as NW
    from sonet_hip import synth
    B, N, steps, P = 8, 5000, 6, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--batch", str(B),
           "--in-flight", str(P), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["in_flight"] == P and line["value"] > 0 and line["ms_per_step"] > 0
    for key in ("kernels", "parity_checked", "other_configs", "cpu_baseline", "summary"):
        assert key not in line, key
    score = np.load(os.path.join(str(tmp_path), "score.npy"))
    assert score.dtype == np.float32 and score.shape == (B, 40)
    dev = torch.device("cuda", 0)
    opt = bench.make_opt(dev, B, N)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    enc.want_first_pn_out = False
    synth.fill_state_dict_(enc.state_dict(), 0)
    synth.fill_state_dict_(cls.state_dict(), 1)
    enc.to(dev).eval()
    cls.to(dev).eval()
    inp = synth.make_inputs(B, N, seed=100 + 1000 * ((steps - 1) % P), device=dev)
    with torch.no_grad():
        want = cls(enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=False)).float().cpu().numpy()
    assert np.array_equal(score, want), float(np.abs(score - want).max())
