"""bench.py -- point-clouds/sec forward, ModelNet40 5k-pt 8x8 SOM (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W         (N > 1: launched by torch.distributed.run)
    python bench.py --gpus N --steps K --warmup W --full  (the headline plus every figure and check below)

A plain run sets up, spins up, warms up, times the K steps and prints the result line (`value`, `ms_per_step`, ...);
--dump-outputs DIR also writes what the last timed step computed.  Everything else -- further windows, the single-stream
figure, per-kernel rooflines, the oracle parity check, the other BASELINE configs and arithmetics, the CPU baseline -- runs
with --full only.

A "step" is one forward pass of the SO-Net ModelNet40 classifier (level-2 Encoder + Classifier
head, eval mode) over one batch of synthetic clouds already resident in HBM: B clouds per GPU,
5000 points, 8x8 SOM, k=3, som_k=9, surface normals on (BASELINE.json configs[1] shape; forward is
the metric).  The batch is sharded over ranks with no data-path collective ("weak" scaling: per-GPU
work fixed).  W untimed warm-up steps, then exactly K steps bracketed by barrier +
torch.cuda.synchronize(); the time is the MAX over ranks; rank 0 prints ONE JSON line.  Before the W warm-up steps every
timed region runs --spin-up seconds (default 1 s, reported as `spin_up`) of untimed steps: an idle MI355X sits at 94 MHz
and reaches its clocks after 0.3-0.5 s of load (profiles/r04y_first_process.log: 3 % on a 20-step window, 40 % on the
first 40 training steps of a fresh box).

Extra objects on the line of a --full run (task contract (4)):
  roofline      -- for the dominant kernel of the step (largest share of kernel time): algorithmic
                   flops (or bytes) per launch / its mean launch duration, measured live with HIP
                   events recorded on the launch stream inside the timed region.
  kernels       -- the same figure for every hand-written kernel of the step.
  cpu_baseline  -- the CPU oracle (oracle/cpu_oracle.py: C restatement + the reference's own compiled
                   index_max + the aten CPU calls the reference makes) timed on this box's host
                   cores on a bounded sample of the same workload (rank 0, N=1 only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "so-net_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
PEAK_VALU_TLANEOPS = 39.3    # 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz: vector instructions x lanes per second, in 1e12
PEAK_F32_MFMA_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # v_mfma_f32_32x32x16_bf16, dense
# the 3xbf16-split path issues 6 bf16 MFMAs per algorithmic f32 product: its ceiling in algorithmic flops
PEAK_X3_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0
# the fused first PointNet splits into fp16 pieces and issues 3 fp16 MFMAs (same 2.5 PF dense rate) per product
PEAK_H3_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 3.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)         # (a step is ~1 ms: the whole default run stays well under a minute)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64, help="clouds per GPU (BASELINE configs[4]: 512 / 8 GPUs)")
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--precision", choices=["h3", "x3", "f32", "bf16"], default=None,
                    help="point-wise layer arithmetic: h3 = three-term fp16 split (default, f32-class, parity 1e-5), x3 = 3xbf16 split, "
                         "f32 = exact f32 MFMA, bf16 = bf16 storage + one bf16 MFMA per product (BASELINE configs[1]; reduced precision)")
    ap.add_argument("--mode", choices=["forward", "train"], default="forward",
                    help="forward = the BASELINE metric (default); train = forward+backward+gradient all-reduce+Adam "
                         "(BASELINE configs[4], reported under its own metric name)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a HIP graph")
    ap.add_argument("--in-flight", type=int, default=4,   # (3 -> 4: +2 % in three interleaved A/B pairs on two boxes, 5 and 6: no better -- docs/findings.md R6.2)
                    help="independent batches in flight: P HIP graphs replayed round-robin on P streams (1 = one stream; forward mode)")
    ap.add_argument("--cpu-clouds", type=int, default=8, help="clouds in the CPU-baseline sample")
    ap.add_argument("--no-other-precisions", action="store_true", help="skip the x3 / exact-f32 throughput keys")
    ap.add_argument("--no-parity-check", action="store_true", help="skip the oracle check of the timed batch (rank 0)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the other BASELINE.json configs (training step bf16 / f32-class, segmenter, autoencoder + Chamfer) under `other_configs`")
    ap.add_argument("--other-steps", type=int, default=30, help="timed steps per window of each `other_configs` entry")
    ap.add_argument("--only-other", default="", help="comma-separated substrings: run only the `other_configs` entries whose name contains one (experiments)")
    ap.add_argument("--windows", type=int, default=3, help="timed windows of K steps of the headline (the first one is `value`)")
    ap.add_argument("--range-check-every", type=int, default=None,
                    help="period (replays) of the non-blocking operand-range check of the replayed graphs (default: sonet_hip.graph.CHECK_EVERY; 0 = off)")
    ap.add_argument("--spin-up", type=float, default=1.0,
                    help="seconds of untimed steps before the W warm-up steps of a timed region: an idle MI355X sits at 94 MHz and needs "
                         "0.3-0.5 s of load to reach its clocks (tools/first_process.py); 0 = none")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: further windows, single-stream figure, per-kernel rooflines, oracle parity check, "
                         "other BASELINE configs, other arithmetics, CPU baseline (the --no-* options and --windows / --other-steps refine it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32; rank 0's shard)")
    return ap.parse_args()


def dump_outputs(path, arrays):
    """Write each array as path/<name>.npy in float32 (the caller passes what its timed path hands back, well under 64 MB)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.detach().float().cpu().numpy())


def spawn_ranks(args):
    """``python bench.py --gpus N`` without a torch.distributed.run environment: launch the N ranks ourselves (the same
    command line the driver uses) and hand back their exit code.  Fails loudly when fewer than N GPUs are visible."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < args.gpus:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node; refusing to report a smaller job as %d GPUs"
                         % (args.gpus, have, args.gpus))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


BF16_TOL = 5e-2     # bf16 storage: worst element within 5e-2 * max(|ref|, rms(ref)) of the f32 oracle (tests/test_gpu_bf16.py)


def parity_check(args, enc, cls, inp, out, enc_sd, cls_sd, n_clouds=4):
    """The oracle on the first clouds of the TIMED batch vs what the timed path produced for them: node ids bit-exact,
    feature / score within 1e-5 * max(|ref|, rms(ref)) -- so the number on the line belongs to results that were checked."""
    _assert_untimed('parity_check')
    import numpy as np
    from oracle import cpu_oracle as O
    P = min(n_clouds, args.batch)
    with torch.no_grad():
        feat = enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=False)   # eager twin of the replayed step
        score_eager = cls(feat)
    got_idx = enc.min_idx[:P].cpu().numpy()
    ref = O.encoder_forward(enc_sd, inp["pc"][:P].cpu(), inp["sn"][:P].cpu(), inp["node"][:P].cpu(), inp["node_knn_I"][:P].cpu(),
                            use_ref_index_max=O.ref_module() is not None)
    ref_score = O.classifier_forward(cls_sd, ref["feature"])

    from sonet_hip import ops as _o
    tol = BF16_TOL if _o.POINTMLP_PRECISION == "bf16" else 1e-5

    def worst(a, b):
        a, b = a.detach().cpu().double().numpy(), b.detach().double().numpy()
        bound = tol * np.maximum(np.abs(b), np.sqrt(np.mean(b ** 2)))
        return float((np.abs(a - b) / bound).max())

    # node ids of EVERY cloud of the timed batch against the C restatement of BatchSOM.query_topk (util/som.py:237-269)
    all_idx = enc.min_idx.cpu().numpy()
    ids_ok = bool(np.array_equal(all_idx, O.som_query_topk(inp["pc"].cpu(), inp["node"].cpu(), int(enc.opt.k))[0]))
    res = {"clouds": P, "of_the_timed_batch": True, "min_idx_bit_exact": bool(np.array_equal(got_idx, ref["min_idx"])),
           "node_ids_bit_exact_all_clouds": {"clouds": args.batch, "ok": bool(ids_ok)},
           "feature_err_over_bound": round(worst(feat[:P], ref["feature"]), 4),
           "score_err_over_bound": round(worst(out[:P], ref_score), 4),
           "replay_equals_eager": bool(torch.equal(out, score_eager)),
           "bound": "%g * max(|ref|, rms(ref))" % tol, "oracle": "oracle/cpu_oracle.py"}
    res["ok"] = bool(res["min_idx_bit_exact"] and ids_ok and res["feature_err_over_bound"] <= 1.0 and res["score_err_over_bound"] <= 1.0)
    if not res["ok"]:
        raise SystemExit("bench.py: the timed batch does NOT match the oracle: %s" % json.dumps(res))
    return res


def make_opt(dev, B, N):
    from argparse import Namespace
    return Namespace(gpu_id=dev.index or 0, device=dev, batch_size=B, input_pc_num=N, surface_normal=True,
                     feature_num=1024, activation="relu", normalization="batch", dropout=0.7, node_num=64, k=3,
                     som_k=9, som_k_type="avg", bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6,
                     classes=40)


def algorithmic(name, B, N, k=3, M=64, C=384):
    """(kind, amount per launch): algorithmic bytes for the HBM-bound kernels, flops for the MFMA ones
    (per-cloud figures of SURVEY.md 8(d) / DESIGN.md x the B clouds one launch processes)."""
    kN = k * N
    if name == "index_max_gather":
        return "hbm", B * (C * kN * 4 + kN * 4 + 2 * C * M * 4 + M * 4)
    if name == "index_max":
        return "hbm", B * (C * kN * 4 + kN * 4 + C * M * 4)
    if name == "som_assign":
        return "hbm", B * (3 * N * 4 + 3 * M * 4 + kN * 4 + M * 4 + 3 * M * 8)
    if name == "som_assign_sort":                              # assignment (x, nodes -> ids) + node-sorted grouping (x, sn, ids -> 6 sorted planes + ids)
        return "hbm", B * (3 * N * 4 + 3 * M * 4 + kN * 4 + M * 4) + B * (6 * N * 4 + kN * 4 + 6 * kN * 4 + kN * 4 + 3 * M * 4 + 2 * M * 4)
    if name == "som_group":
        return "hbm", B * (6 * N * 4 + kN * 4 + M * 4 + 3 * M * 8 + 6 * kN * 4 + 3 * M * 4 + M * 4)
    if name == "knn_gather":
        return "hbm", None
    if name.startswith("pointresnet_"):
        L = int(name.split("_L")[1])
        return "mfma", 2.0 * (6 * 64 + 64 * 128 + 128 * 256 + 320 * 384) * B * L
    if name.startswith("pointmlp"):
        dims, L = name.split("_", 1)[1].split("_L")
        cin, cout = dims.split("_")[-1].split("x")              # (pointmlph3_nodeadd_393x1024_L3072: a variant tag in front of the dims)
        if "_flat_" in name or "_gmax" in name:                 # flat node-level stage: ONE cloud whose L columns already span the batch
            B = 1
        if name.startswith("pointmlpbf16_pool"):                # the layer whose epilogue is the pool: nothing written, the input once -- bound by the matrix pipe
            return "mfma", 2.0 * int(cin) * int(cout) * B * int(L.split("_")[0])
        if name.startswith("pointmlpbf16"):                     # one bf16 MFMA per product: 175 flop per byte at 320 -> 384, under the machine balance
            return "hbm", 2.0 * (int(cin) + int(cout)) * B * int(L.split("_")[0])    # input + output, once, 2 bytes each
        return "mfma", 2.0 * int(cin) * int(cout) * B * int(L.split("_")[0])     # ("_kmax9": the max over k is in the epilogue)
    return "hbm", None


def cpu_baseline(args, enc_sd, cls_sd):
    """Oracle forward on the host cores, bounded sample (about 10-30 s)."""
    _assert_untimed('cpu_baseline')
    from oracle import cpu_oracle as O
    from sonet_hip import synth
    ncpu = os.cpu_count() or 1
    Bc = args.cpu_clouds
    inp = synth.make_inputs(Bc, args.points, seed=1234)
    use_ref = O.ref_module() is not None

    def run(threads):
        r = O.encoder_forward(enc_sd, inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"],
                              index_max_threads=threads, use_ref_index_max=use_ref)
        return O.classifier_forward(cls_sd, r["feature"])

    # all host cores is rarely the fastest for these small convolutions: try a few thread counts within
    # the time bound and report the best (cores = the thread count of the reported number)
    best, cores, reps = float("inf"), 1, 0
    with torch.no_grad():
        for threads in sorted({min(ncpu, 8), min(ncpu, 32), ncpu}):
            torch.set_num_threads(threads)
            run(threads)                                     # warm-up
            t_start = time.perf_counter()
            for _ in range(3):
                t0 = time.perf_counter()
                run(threads)
                dt = time.perf_counter() - t0
                reps += 1
                if dt < best:
                    best, cores = dt, threads
                if time.perf_counter() - t_start > 8.0:
                    break
    return {"value": Bc / best, "unit": "clouds/s", "cores": cores, "kind": "port",
            "sample": "%d clouds x %d pts, full classifier forward (oracle/cpu_oracle.py: C restatement of the SOM "
                      "assignment/grouping, %s index_max with %d threads, aten CPU conv/BN as the reference calls), "
                      "best of %d timed runs over thread counts {8, 32, all=%d}" % (Bc, args.points,
                                                       "the reference's own compiled" if use_ref else "restated", cores, reps, ncpu)}


def rank_evidence(world, rank, dev, my_clouds_per_s):
    """Every rank reports the physical device it ran on (UUID, PCI bus id) and its own clouds/s; rank 0 puts the list on the
    line and FAILS the run when two ranks sat on the same device -- an N-GPU number cannot come from fewer than N GPUs."""
    pr = torch.cuda.get_device_properties(dev)
    me = {"rank": rank, "local_device": dev.index, "name": pr.name, "uuid": str(getattr(pr, "uuid", "")),
          "pci": "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0), getattr(pr, "pci_device_id", 0)),
          "clouds_per_s": round(my_clouds_per_s, 1)}
    if world > 1:
        allr = [None] * world
        torch.distributed.all_gather_object(allr, me)
    else:
        allr = [me]
    ids = [(r_["uuid"], r_["pci"]) for r_ in allr]
    distinct = len(set(ids))
    if distinct != world:
        raise SystemExit("bench.py: %d ranks ran on %d distinct device(s): %s" % (world, distinct, ids))
    rates = [r_["clouds_per_s"] for r_ in allr]
    return {"world": world, "distinct_devices": distinct, "per_rank_clouds_per_s": {"min": min(rates), "max": max(rates)}, "devices": allr}


def _kernel_top(rec, steps, B, N, n=5):
    """Top kernels of an instrumented region (ops.kernel_timing) + the roofline of the dominant one that has an
    algorithmic figure (same convention as the headline's `roofline`)."""
    summ = rec.summary()
    tot = sum(v["total_ms"] for v in summ.values()) or 1.0
    top, roof = [], None
    for name, s_ in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"]):
        e = {"name": name, "ms_per_step": round(s_["total_ms"] / steps, 4), "share": round(s_["total_ms"] / tot, 3)}
        try:
            bound, amount = algorithmic(name, B, N)
        except Exception:
            bound, amount = None, None
        if amount and roof is None:
            if bound == "mfma":
                peak = (PEAK_H3_TFLOPS if name.startswith(("pointresnet_fused", "pointmlph3", "pointmlpws")) else PEAK_X3_TFLOPS if name.startswith("pointmlpx3")
                        else PEAK_BF16_MFMA_TFLOPS if name.startswith(("pointresnet_bf16", "pointmlpbf16")) else PEAK_F32_MFMA_TFLOPS)
                ach = amount / (s_["mean_ms"] * 1e-3) / 1e12
                roof = {"kernel": name, "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                        "mean_ms": round(s_["mean_ms"], 5)}
            else:
                ach = amount / (s_["mean_ms"] * 1e-3) / 1e9
                roof = {"kernel": name, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4),
                        "mean_ms": round(s_["mean_ms"], 5)}
        if len(top) < n:
            top.append(e)
    return top, roof


def _encoder_parity(enc, inp, P=2, tol=1e-5, **kw):
    """The encoder stage of a timed batch against the oracle on its first P clouds (node ids bit-exact, feature within tol)."""
    _assert_untimed('_encoder_parity')
    import numpy as np
    from oracle import cpu_oracle as O
    sd = {k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
    ref = O.encoder_forward(sd, inp["pc"][:P].cpu(), inp["sn"][:P].cpu(), inp["node"][:P].cpu(), inp["node_knn_I"][:P].cpu(),
                            use_ref_index_max=O.ref_module() is not None, **kw)
    b = ref["feature"].double().numpy()
    a = enc.feature[:P].detach().cpu().double().numpy()
    bound = tol * np.maximum(np.abs(b), np.sqrt(np.mean(b ** 2)))
    res = {"clouds": P, "min_idx_bit_exact": bool(np.array_equal(enc.min_idx[:P].cpu().numpy(), ref["min_idx"])),
           "feature_err_over_bound": round(float((np.abs(a - b) / bound).max()), 4), "bound": "%g * max(|ref|, rms(ref))" % tol,
           "oracle": "oracle/cpu_oracle.py encoder_forward"}
    res["ok"] = bool(res["min_idx_bit_exact"] and res["feature_err_over_bound"] <= 1.0)
    return res


def make_adam(module):
    """The reference's optimizer (models/classifier.py:45-49: Adam, lr 1e-3, betas (0.9, 0.999)) -- as sonet_hip.optim.FusedAdam, the same
    update in one launch (tests/test_gpu_optim.py pins it against torch.optim.Adam); SONET_TORCH_ADAM=1 times torch.optim.Adam itself."""
    if os.environ.get("SONET_TORCH_ADAM", "0") == "1":
        return torch.optim.Adam(module.parameters(), lr=1e-3, betas=(0.9, 0.999))
    from sonet_hip.optim import FusedAdam
    return FusedAdam(module.parameters(), lr=1e-3, betas=(0.9, 0.999))


_TIMED = [0]          # > 0 while a timed window is open on this rank: the CPU oracle (32 threads on rank 0) must never run then


class _timed_region:
    def __enter__(self):
        _TIMED[0] += 1

    def __exit__(self, *exc):
        _TIMED[0] -= 1
        return False


def _assert_untimed(what):
    if _TIMED[0]:
        raise SystemExit("bench.py: %s (CPU oracle) called inside a timed window" % what)


def pin_host_threads(world, local_rank):
    """A job of several ranks shares one host: give every rank its own contiguous block of the cores this process may use (contiguous =
    NUMA-local on the two-socket boxes) and size torch's intra-op pool to it, so that one rank's host work -- rank 0's oracle legs
    between the timed windows, the Python enqueue loop of the training step -- cannot land on another rank's launch thread."""
    if world <= 1 or not hasattr(os, "sched_getaffinity"):
        return None
    cpus = sorted(os.sched_getaffinity(0))
    per = len(cpus) // world
    if per < 1:
        return None
    mine = cpus[local_rank * per:(local_rank + 1) * per]
    try:
        os.sched_setaffinity(0, mine)
    except OSError:
        return None
    torch.set_num_threads(max(1, min(32, per)))
    return {"cpus_per_rank": per, "first": mine[0], "last": mine[-1], "torch_threads": torch.get_num_threads()}


def _windows(fn, steps, n=3, dev=None, collective=False):
    """n timed windows of `steps` calls.  collective (a job of several ranks): a barrier on both sides of every window and the MAX over
    ranks, as for the headline; returns (seconds per step of the job, seconds per step of this rank)."""
    from sonet_hip import dp
    ts, mine = [], []
    for _ in range(n):
        if collective:
            dp.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with _timed_region():
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        me = (time.perf_counter() - t0) / steps
        if collective:
            dp.barrier()
            torch.cuda.synchronize()
            ts.append(dp.all_reduce_max((time.perf_counter() - t0) / steps, dev))
        else:
            ts.append(me)
        mine.append(me)
    return ts, mine


def _spin_up(fn, seconds, chunk=16, dev=None, sync=None):
    """Untimed calls of `fn` for `seconds` of wall time (device drained every `chunk` calls): clocks up before a timed region.
    Returns the number of calls.  In a job of several ranks `fn` may contain collectives (the gradient all-reduce of the training step):
    every rank must make the SAME number of calls, so the decision to go on is taken on the MAX of the ranks' clocks (one small
    all-reduce per chunk).  Also: sonet_hip.host.freeze_gc() -- a generation-2 pass of CPython's cyclic collector over the ~270,000
    objects of a torch process takes 70 ms, more than three 20-step windows of the headline (profiles/r04y_gc_pause.log)."""
    from sonet_hip import dp, host
    host.freeze_gc()
    n, t0 = 0, time.perf_counter()
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev     # (dev / sync: the gloo test of the rank agreement)
    sync = torch.cuda.synchronize if sync is None else sync
    while seconds > 0 and dp.all_reduce_max(time.perf_counter() - t0, dev) < seconds:
        for _ in range(chunk):
            fn()
        sync()
        n += chunk
    return n


def other_configs(args, dev, world=1, rank=0):
    """world > 1 (the driver's --gpus N command, EVERY rank calls this): BASELINE configs[4] -- the data-parallel training step, global
    batch 64 x N, bucketed RCCL gradient all-reduce -- in bf16 and in the f32-class arithmetic, timed like the headline (barrier on both
    sides, max over ranks); returns the entries on rank 0, None elsewhere.  world == 1:
    the other BASELINE.json configs on one GPU, after the headline (same process, inputs resident, >= 30 timed steps per
    window, three windows, the median reported): configs[1] the 5000-point classifier TRAINING step in bf16 and in the f32-class
    arithmetic (models/classifier.py:78-99), configs[2] the part segmenter at 1024 points (models/segmenter.py:79-109),
    configs[3] the autoencoder forward with the Chamfer loss (models/autoencoder.py:66-103).  Each entry carries the roofline of
    its dominant kernel and an oracle check of its timed batch.  A failing entry is reported, never hidden."""
    from argparse import Namespace
    from models import networks as NW, losses as LS
    from sonet_hip import dp, ops, synth
    from sonet_hip.graph import GraphedForward
    K = max(1, args.other_steps)
    out = {}

    only = [w for w in getattr(args, "only_other", "").split(",") if w]

    def guarded(name, fn):
        if only and not any(w in name for w in only):
            return
        t0 = time.perf_counter()
        try:
            out[name] = fn()
        except Exception as e:                                   # noqa: BLE001 -- the headline must still be printed
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        out[name]["wall_s"] = round(time.perf_counter() - t0, 1)
        # (every entry starts from an empty allocator cache: the blocks a previous entry's model left cached are of no use to the next)
        torch.cuda.empty_cache()

    def train(precision):
        B, N = args.batch, args.points
        with ops.precision(precision):
            opt = make_opt(dev, B, N)
            enc, cls = NW.Encoder(opt), NW.Classifier(opt)
            enc.want_first_pn_out = False                         # (a classifier: nobody reads first_pn_out per point copy)
            synth.fill_state_dict_(enc.state_dict(), 0)
            synth.fill_state_dict_(cls.state_dict(), 1)
            enc.to(dev).train()
            cls.to(dev).train()
            inp = synth.make_inputs(B, N, seed=100 + rank, device=dev)     # this rank's shard of the global batch
            dp.init_distributed(force=True)                       # (world 1: a one-rank RCCL group, the same bucketed exchange as the 8-GPU job)
            dp.broadcast_parameters([enc, cls])
            opt_e, opt_c = make_adam(enc), make_adam(cls)
            reducer = dp.GradientAllReducer([enc, cls], always_reduce=True)
            state = {}

            def step():
                feat = enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=True, epoch=0)
                score = cls(feat, 0)
                enc.zero_grad(set_to_none=True)
                cls.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(score, inp["label"])
                loss.backward()
                state["nbytes"] = reducer.reduce()
                opt_e.step()
                opt_c.step()
                state["loss"] = loss
            # the batch that is about to be timed, eval forward with the initial weights, against the oracle (gates `ok`; rank 0's shard)
            par = None
            if rank == 0:
                enc.eval()
                with torch.no_grad():
                    enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=False)
                par = _encoder_parity(enc, inp, 2, tol=BF16_TOL if precision == "bf16" else 1e-5)
                enc.train()
            _spin_up(step, 0.5 * args.spin_up, chunk=8)
            for _ in range(5):
                step()
            ts, mine = _windows(step, K, dev=dev, collective=world > 1)
            exposed_us = reducer.exposed_ms(last=K) * 1e3
            assert torch.isfinite(state["loss"])
            with ops.kernel_timing() as rec:
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
            top, roof = _kernel_top(rec, 3, B, N)
            reducer.remove_hooks()
            my_med = sorted(mine)[len(mine) // 2]
            per_rank = [my_med]
            if world > 1:
                per_rank = [None] * world
                torch.distributed.all_gather_object(per_rank, my_med)
            if rank != 0:
                return None
            # the model that was just trained, in eval mode, against the oracle with the SAME (updated) weights
            enc.eval()
            with torch.no_grad():
                enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=False)
            tol = BF16_TOL if precision == "bf16" else 1e-5
            after = _encoder_parity(enc, inp, 2, tol=tol)
            # ~100 Adam steps on random labels overfit the 64 clouds and leave a WORSE-CONDITIONED network behind (the folded BatchNorm scale
            # of the first layer grows 2 -> 5.7, running variances fall 0.5 -> 0.06: tools/bf16_drift.py, profiles/r04i_bf16_drift.log), so every
            # arithmetic is further from the oracle than on the fixtures' weights -- the f32-class forward too (3.6e-6 -> 1.0e-5).  What the
            # step must preserve is the ARITHMETIC: the same weights in the f32-class arithmetic give the conditioning, and the bf16 error
            # must stay within the ratio of the unit roundoffs of that (2^-9 / 2^-22 = 2^13, gated at 2^14); node ids stay bit-exact.
            gate = {"min_idx_bit_exact": after["min_idx_bit_exact"], "feature_err_over_bound": after["feature_err_over_bound"]}
            if precision == "bf16":
                with torch.no_grad(), ops.precision("h3"):
                    enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=False)
                ref32 = _encoder_parity(enc, inp, 2, tol=1e-5)
                ratio = (after["feature_err_over_bound"] * tol) / max(ref32["feature_err_over_bound"] * 1e-5, 1e-12)
                # The RATIO below is reported, not gated: the figure is the bf16 feature error on weights ~100 Adam steps on random labels left behind -- a
                # worse-conditioned network (the first layer's folded BatchNorm scale 2 -> 5.7, running variances 0.5 -> 0.06:
                # tools/bf16_drift.py), on which the f32-class arithmetic is further from the oracle too.  A ratio to that error is an
                # explanation, not a bound (a 14 % feature error would pass a 2^14 ratio), so no pass/fail is derived from it: the gate
                # of this entry is the node ids (bit-exact) plus the `before` check above on the fixtures' weights at the stated tolerance.
                # What IS gated (`ok` must not be blind to a regression of the bf16 numerics after training): a loose absolute
                # ceiling of 4 x the fixtures' bound -- the f32-class entries' ceiling -- on the feature error itself (measured 1.4 x).
                gate.update(f32_class_same_weights_err_over_1e5_bound=ref32["feature_err_over_bound"], bf16_over_f32_class_error=round(ratio, 1),
                            gated=True, ceiling_over_bound=4.0, ok=bool(after["min_idx_bit_exact"] and after["feature_err_over_bound"] <= 4.0))
            else:
                gate.update(gated=True, ok=bool(after["min_idx_bit_exact"] and after["feature_err_over_bound"] <= 4.0))
            gate["what"] = ("the same check with the weights and BatchNorm running statistics the timed Adam steps left behind (random labels, %d steps: "
                            "a worse-conditioned network, see tools/bf16_drift.py).  f32-class: gated at node ids bit-exact and features within 4 x the "
                            "fixtures' bound.  bf16: node ids bit-exact and features within 4 x the fixtures' bf16 bound (a loose ceiling: the ratio to the "
                            "f32-class error on the same weights is reported beside it, as an explanation, not a bound)" % (5 + 3 * K + 3))
            par["after_the_timed_steps"] = gate
            par["ok"] = bool(par["ok"] and gate["ok"])
            med = sorted(ts)[len(ts) // 2]
            return {"workload": "ModelNet40 classifier TRAINING step (forward + backward + gradient all-reduce + Adam), %d rank(s) x %d x %d pts" % (world, B, N),
                    "arithmetic": precision, "n_gpus": world, "batch_per_gpu": B, "global_batch": B * world,
                    "clouds_per_s": round(world * B / med, 1), "ms_per_step": round(med * 1e3, 4),
                    "ms_per_step_windows": [round(t * 1e3, 4) for t in ts], "steps_per_window": K,
                    "per_rank_ms_per_step": {"min": round(min(per_rank) * 1e3, 4), "max": round(max(per_rank) * 1e3, 4),
                                             "what": "each rank's own median window, without the closing barrier"},
                    "allreduce": {"backend": torch.distributed.get_backend(), "rccl_world_size": torch.distributed.get_world_size(),
                                  "bytes_per_step": state["nbytes"], "buckets": len(reducer.buckets), "exposed_us_per_step": round(exposed_us, 1)},
                    "top_kernels": top, "roofline": roof,
                    "loss_after": round(float(state["loss"].detach()), 5),
                    "parity_checked": dict(par, what="eval forward of the timed batch with the weights the timed steps start from vs the oracle; "
                                                "training gradients are pinned by tests/golden/train_step_* (tests/test_gpu_parity.py, tests/test_gpu_bf16.py)")}

    def heads_opt(B, N, **kw):
        d = dict(gpu_id=dev.index or 0, device=dev, batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                 normalization="batch", dropout=0.6, node_num=64, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                 bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=50, output_fc_pc_num=256, output_conv_pc_num=1024)
        d.update(kw)
        return Namespace(**d)

    def graphed(fwd, inp, B, N, workload, parity):
        with torch.no_grad():
            g = GraphedForward(fwd, (inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"]), warmup=3)
            call = lambda: g(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])     # noqa: E731
            for _ in range(3):
                call()
            _spin_up(call, 0.5 * args.spin_up)
            ts, _ = _windows(call, K)
            bad = g.range_violations()
            for _ in range(2):
                fwd(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])
            torch.cuda.synchronize()
            with ops.kernel_timing() as rec:
                for _ in range(3):
                    fwd(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])
                torch.cuda.synchronize()
        top, roof = _kernel_top(rec, 3, B, N)
        med = sorted(ts)[len(ts) // 2]
        return {"workload": workload, "arithmetic": ops.POINTMLP_PRECISION, "launch_mode": "hip-graph replay, one stream",
                "clouds_per_s": round(B / med, 1), "ms_per_step": round(med * 1e3, 4), "ms_per_step_windows": [round(t * 1e3, 4) for t in ts],
                "steps_per_window": K, "range_guard_violations": len(bad), "top_kernels": top, "roofline": roof, "parity_checked": parity()}

    def segmenter():
        B, N = args.batch, 1024
        opt = heads_opt(B, N, som_k_type="center")
        enc, seg = NW.Encoder(opt), NW.Segmenter(opt)
        synth.fill_state_dict_(enc.state_dict(), 1)
        synth.fill_state_dict_(seg.state_dict(), 2)
        enc.to(dev).eval()
        seg.to(dev).eval()
        inp = synth.make_inputs(B, N, seed=3, device=dev)
        label = torch.randint(0, 16, (B,), device=dev)
        fwd = lambda pc, sn, node, knn: NW.segmentation_forward(enc, seg, pc, sn, label, node, knn)     # noqa: E731

        def parity():
            r = _encoder_parity(enc, inp, 2, som_k_type="center")
            r["what"] = ("encoder stage of the timed batch vs the oracle; the per-point head (node_gather back-broadcast + 3356-channel "
                         "layer) is pinned by tests/golden/segmenter_b2_n{256,1024} written from the live reference")
            return r
        return graphed(fwd, inp, B, N, "ShapeNetPart segmenter forward (encoder + per-point head, eval), %d x %d pts, 50 parts" % (B, N), parity)

    def autoencoder():
        import numpy as np
        from oracle import cpu_oracle as O
        B, N = args.batch, args.points
        opt = heads_opt(B, N, classes=40)
        enc, dec, crit = NW.Encoder(opt), NW.Decoder(opt), LS.ChamferLoss(opt)
        synth.fill_state_dict_(enc.state_dict(), 1)
        synth.fill_state_dict_(dec.state_dict(), 2)
        enc.to(dev).eval()
        dec.to(dev).eval()
        inp = synth.make_inputs(B, N, seed=3, device=dev)
        keep = {}

        def fwd(pc, sn, node, knn):
            pred = dec(enc(pc, sn, node, knn, False, None))
            keep["pred"], keep["conv"] = pred, dec.conv_pc4
            return crit(pred, pc) + crit(dec.conv_pc4, pc)

        def parity():
            r = _encoder_parity(enc, inp, 2)
            with torch.no_grad():
                pred = dec(enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], False, None))
                got = float(crit(pred[:2], inp["pc"][:2]))
            f, b, _ = O.chamfer_loss(pred[:2].cpu().numpy(), inp["pc"][:2].cpu().numpy())
            rel = abs(got - (f + b)) / max(abs(f + b), 1e-30)
            r.update(chamfer_loss={"got": got, "oracle": f + b, "rel_err": float(rel), "ok": bool(rel <= 1e-5),
                                   "what": "Chamfer loss of the decoder output for 2 clouds vs oracle chamfer_loss (models/losses.py:237-290 restated; "
                                           "exact brute-force 1-NN stands in for faiss: parity unpinned at that boundary)"})
            r["ok"] = bool(r["ok"] and rel <= 1e-5)
            return r
        return graphed(fwd, inp, B, N, "autoencoder forward (encoder + decoder + two-resolution Chamfer loss, eval), %d x %d pts vs %d + %d predicted"
                       % (B, N, 256 + 1024, 1024), parity)

    if world > 1:
        # (no exception guard: a rank that failed alone would leave the others waiting in the next collective)
        for precision in ("bf16", "h3"):
            t0 = time.perf_counter()
            e = train(precision)
            if e is not None:
                out["configs[4] train %s" % precision] = dict(e, wall_s=round(time.perf_counter() - t0, 1))
        return out if rank == 0 else None
    guarded("configs[1] train bf16", lambda: train("bf16"))
    guarded("configs[1] train h3", lambda: train("h3"))
    guarded("configs[2] segmenter", segmenter)
    guarded("configs[3] autoencoder", autoencoder)
    return out


def train_bench(args, enc, cls, inp, world, rank, dev):
    """Data-parallel training step (models/classifier.py:78-99 + the bucketed RCCL gradient all-reduce of sonet_hip/dp.py)."""
    from sonet_hip import dp
    enc.train()
    cls.train()
    dp.broadcast_parameters([enc, cls])
    opt_e, opt_c = make_adam(enc), make_adam(cls)
    # always_reduce: the RCCL collectives run even in a single-rank group, so the 1-GPU line exercises (and prices) the same
    # hook-driven bucketed exchange the 8-GPU job uses
    reducer = dp.GradientAllReducer([enc, cls], always_reduce=torch.distributed.is_initialized())
    label = inp["label"]

    def step():
        feat = enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=True, epoch=0)
        score = cls(feat, 0)
        enc.zero_grad(set_to_none=True)      # (no fill launch per parameter; backward assigns instead of accumulating)
        cls.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(score, label)
        loss.backward()
        nbytes = reducer.reduce()
        opt_e.step()
        opt_c.step()
        return loss, nbytes

    # The spin-up runs for a wall time, not a number of steps, and every step moves the weights, the optimizer moments, the BatchNorm
    # statistics and the dropout generator: the warm-up and timed steps start from the state before it, so that their inputs are the
    # same in every run with the same arguments (--dump-outputs).  (Their outputs are not bit-reproducible: the BatchNorm-backward
    # channel sums are float atomics, and Adam turns last-bit differences of small gradients into lr-sized ones.)
    start = [{k: v.clone() for k, v in m.state_dict().items()} for m in (enc, cls)]
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    _spin_up(step, args.spin_up, chunk=8)
    torch.cuda.synchronize()
    with torch.no_grad():
        for m, sd in zip((enc, cls), start):
            for k, v in m.state_dict().items():
                v.copy_(sd[k])
    del start
    torch.set_rng_state(rng[0])
    torch.cuda.set_rng_state(rng[1], dev)
    opt_e, opt_c = make_adam(enc), make_adam(cls)
    for _ in range(max(1, args.warmup)):
        loss, nbytes = step()
    dp.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with _timed_region():
        for _ in range(args.steps):
            loss, nbytes = step()
        dp.barrier()
        torch.cuda.synchronize()
    my_elapsed = time.perf_counter() - t0
    elapsed = dp.all_reduce_max(my_elapsed, dev)
    assert torch.isfinite(loss)
    exposed_us = reducer.exposed_ms(last=args.steps) * 1e3
    ranks = rank_evidence(world, rank, dev, args.batch * args.steps / my_elapsed)
    if rank != 0:
        return
    if args.dump_outputs:
        # what a caller of the training step ends up with: its loss and the weights / BatchNorm statistics it leaves behind
        flat = lambda m: torch.cat([v.detach().float().reshape(-1) for v in m.state_dict().values() if v.is_floating_point()])   # noqa: E731
        dump_outputs(args.dump_outputs, {"loss": loss, "encoder_state": flat(enc), "classifier_state": flat(cls)})
    B, N = args.batch, args.points
    from sonet_hip import ops
    return ({
        "metric": "point-clouds/sec training step (forward+backward+all-reduce+Adam), ModelNet40 5k-pt 8x8 SOM",
        "value": round(world * B * args.steps / elapsed, 2), "unit": "clouds/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / args.steps, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": ("bf16 (bf16 storage of activations and gradients, one bf16 MFMA per product, f32 accumulate, f32 master weights; "
                                       "weight gradients: sonet_wgrad_bf16, bf16 operands -> f32, fixed-order reduction; the two KNN-level ones and 64 x 6 on hipBLASLt)"
                                       if ops.POINTMLP_PRECISION == "bf16"
                                       else "f32 (%s forward -- the first PointNet on node-sorted columns, its last layer pools its own output, hidden activations "
                                            "normalised by their consumers' operand loads --, x3 dgrad; weight gradients: sonet_wgrad_x3, 3 x bf16 split of both "
                                            "operands, fixed-order reduction; 64 x 6 on hipBLASLt f32)" % ops.POINTMLP_PRECISION), "data": "synthetic",
        "config": {"workload": "ModelNet40 classifier training step, %d pts, 8x8 SOM, k=3, som_k=9" % N, "batch_per_gpu": B,
                   "global_batch": B * world, "parallelism": "dp%d: batch shards + %d-byte gradient all-reduce per step in %d bucket(s) started from gradient hooks during backward"
                                  % (world, nbytes, max(1, len(reducer.buckets)))},
        "ranks": ranks,
        "allreduce": {"backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else None,
                      "rccl_world_size": torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1, "bytes_per_step": nbytes,
                      "buckets": len(reducer.buckets), "exposed_us_per_step": round(exposed_us, 1),
                      "what": "GPU time between the last backward kernel and the arrival of the last bucket (HIP events around the waits)"},
        "range_guard": {"enabled": bool(ops.RANGE_GUARD), "arithmetic_at_end": ops.POINTMLP_PRECISION}})


def headline(args, world, rank, dev, elapsed, window_s, P, use_graph, spin_calls, host_pin):
    """The forward metric's result line: every rank calls it (the times are the max over ranks), `value` is the first timed window."""
    from sonet_hip import dp, ops
    B, N = args.batch, args.points
    my_elapsed = elapsed
    elapsed = dp.all_reduce_max(elapsed, dev)
    window_s = [dp.all_reduce_max(w_, dev) for w_ in window_s]
    ranks = rank_evidence(world, rank, dev, B * args.steps / my_elapsed)
    dtype = ("bf16 (bf16 storage, one bf16 MFMA per product, f32 accumulate; features within 5e-2 of the f32 oracle, indices exact)" if ops.POINTMLP_PRECISION == "bf16"
             else "f32 (operands split into fp16 pieces, 3 fp16 MFMAs per product, f32 accumulate; parity 1e-5)" if ops.POINTMLP_PRECISION == "h3"
             else "f32 (3xbf16-split operands on bf16 MFMA, f32 accumulate; parity 1e-5)" if ops.POINTMLP_PRECISION == "x3"
             else "f32 (exact f32 MFMA)")
    line = {
        "metric": "point-clouds/sec forward, ModelNet40 5k-pt 8x8 SOM",
        "value": round(world * B * args.steps / elapsed, 2), "unit": "clouds/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed * 1e3 / args.steps, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": dtype, "data": "synthetic",
        "config": {"workload": "ModelNet40 classifier forward (level-2 Encoder + Classifier head, eval), %d pts, 8x8 SOM, "
                               "k=3, som_k=9, surface normals" % N,
                   "batch_per_gpu": B, "global_batch": B * world, "points": N,
                   "parallelism": "dp%d: batch shards, no data-path collective" % world},
        "launch_mode": ("hip-graph replay, %d independent batches in flight on %d streams" % (P, P) if use_graph and P > 1
                        else "hip-graph replay" if use_graph else "eager"),
        "spin_up": {"seconds": args.spin_up, "untimed_steps": spin_calls,
                    "what": "untimed replays before the W warm-up steps: an idle MI355X sits at its lowest clock and needs 0.3-0.5 s of load to "
                            "leave it (tools/first_process.py, profiles/r04y_first_process.log); --spin-up 0 = none.  Before every timed region "
                            "sonet_hip.host.freeze_gc() (gc.collect + gc.freeze: no 70 ms generation-2 pause of the Python collector inside a window)"},
        "ranks": ranks,
        "host_threads": host_pin if host_pin is not None else {"pinned": False, "what": "one rank: the process keeps the host's cores (the CPU oracle legs run outside every timed window: asserted)"},
        "in_flight": P, "arithmetic": ops.POINTMLP_PRECISION,
    }
    if args.full:
        # (`value` is the FIRST timed window, as the contract says; the windows of one process spread by several per cent -- clocks --, so
        #  the median of all of them is printed next to it)
        line["value_median"] = round(world * B * args.steps / sorted(window_s)[len(window_s) // 2], 2)
        line["windows"] = {"steps_each": args.steps, "clouds_per_s": [round(world * B * args.steps / w_, 1) for w_ in window_s],
                           "min": round(world * B * args.steps / max(window_s), 1),
                           "median": round(world * B * args.steps / sorted(window_s)[len(window_s) // 2], 1),
                           "what": "whole-job clouds/s of every timed window (max over ranks each); `value` is the first"}
    return line


def main():
    args = parse()
    from models import networks as NW
    from sonet_hip import dp, ops, synth

    if args.precision:
        ops.POINTMLP_PRECISION = args.precision
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no GPU visible and there is no CPU fallback")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))            # not under torch.distributed.run: start the N ranks ourselves
    world, rank, local_rank = dp.init_distributed(force=(args.mode == "train"))   # train: a process group even for one rank (RCCL is exercised)
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    host_pin = pin_host_threads(world, local_rank)

    B, N = args.batch, args.points
    opt = make_opt(dev, B, N)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    enc.want_first_pn_out = False                                  # (a classifier: nobody reads first_pn_out per point copy)
    enc_sd = synth.fill_state_dict_(enc.state_dict(), 0)          # identical weights on every rank
    cls_sd = synth.fill_state_dict_(cls.state_dict(), 1)
    enc_cpu = {k: v.clone() for k, v in enc_sd.items()}
    cls_cpu = {k: v.clone() for k, v in cls_sd.items()}
    enc.to(dev).eval()
    cls.to(dev).eval()
    inp = synth.make_inputs(B, N, seed=100 + rank, device=dev)   # this rank's shard, resident in HBM

    def step():
        feat = enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], is_train=False)
        return cls(feat)

    if args.mode == "train":
        return train_bench(args, enc, cls, inp, world, rank, dev)

    # The step is shape-static: replay it as ONE HIP graph (sonet_hip/graph.py).  `value` is timed on the
    # replays; the per-kernel durations for the roofline come from a second, eagerly launched region of
    # the same K steps with HIP events around every C-ABI launch (events cannot be read inside a graph).
    #
    # Batches of a serving / evaluation loop are independent, and most of the step outside the fused first PointNet is short,
    # latency-bound launches that leave CUs idle: with P graphs replayed round-robin on P HIP streams (each with its own batch and
    # its own workspaces) the SOM stage and the node-level stage of one batch run on the CUs the other batch's kernels do not fill.
    # Same kernels, same results (checked below: a replay among others == the replay alone); `single_stream` keeps the P = 1 figure.
    use_graph = not args.no_graph
    P = max(1, args.in_flight) if use_graph else 1
    fwd = lambda pc, sn, node, knn: cls(enc(pc, sn, node, knn, is_train=False))      # noqa: E731
    with torch.no_grad():
        if use_graph:
            from sonet_hip import graph as _graph
            from sonet_hip.graph import GraphedForward
            if args.range_check_every is not None:
                _graph.CHECK_EVERY = max(0, args.range_check_every)
            inps = [inp] + [synth.make_inputs(B, N, seed=100 + rank + 1000 * q, device=dev) for q in range(1, P)]
            graphs = [GraphedForward(fwd, (i_["pc"], i_["sn"], i_["node"], i_["node_knn_I"]), warmup=max(1, args.warmup)) for i_ in inps]
            streams = [torch.cuda.Stream(device=dev) for _ in range(P)]
            graphed = graphs[0]

            def run_many(n, first=0):
                o = None
                for s_ in range(n):
                    q = (first + s_) % P
                    with torch.cuda.stream(streams[q]):
                        i_ = inps[q]
                        o = graphs[q](i_["pc"], i_["sn"], i_["node"], i_["node_knn_I"])
                return o
        else:
            run_many = lambda n, first=0: [step() for _ in range(n)][-1]            # noqa: E731
        spin_calls = _spin_up(lambda: run_many(P), args.spin_up) * P
        run_many(args.warmup)
        dp.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with _timed_region():
            out = run_many(args.steps)
            dp.barrier()
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        # further windows of the same K steps (`value` is the FIRST window, as the contract says; the spread is on the line)
        # (nothing but the barrier between two windows: the first call of any other operator -- the isfinite check below -- loads its code
        #  object, the GPU idles for a millisecond, and the window behind it starts on sagging clocks: 10-12 % low, docs/findings.md R5.11)
        window_s = [elapsed]
        for _ in range(max(0, args.windows - 1) if args.full else 0):
            dp.barrier()
            torch.cuda.synchronize()
            tw = time.perf_counter()
            with _timed_region():
                run_many(args.steps)
                dp.barrier()
                torch.cuda.synchronize()
            window_s.append(time.perf_counter() - tw)
        assert torch.isfinite(out).all()
        # (every window ends with the same step on the same graph: `out` holds the last timed step's scores, rank 0's shard)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, {"score": out})
        if not args.full:
            line = headline(args, world, rank, dev, elapsed, window_s, P, use_graph, spin_calls, host_pin)
            return line if rank == 0 else None
        single = None
        overlap_ok = None
        if use_graph and P > 1:
            # the same K steps on ONE stream (graph 0 only), and: a replay among the others == the replay alone, bit for bit.
            # (A graph is only ever replayed on ITS stream: the same executable graph launched on two streams at once is undefined --
            # on this runtime a "write access to a read-only page" fault.)
            run_many(2 * P)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            with torch.cuda.stream(streams[0]):
                for _ in range(args.steps):
                    graphs[0](inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])
            torch.cuda.synchronize()
            dt1 = time.perf_counter() - t1
            single = {"clouds_per_s": round(B * args.steps / dt1, 1), "ms_per_step": round(dt1 * 1e3 / args.steps, 4)}
            alone = graphs[0].static_output.clone()
            torch.cuda.synchronize()
            run_many(P, first=1)                              # ends with graph 0, after the other P - 1 were launched
            torch.cuda.synchronize()
            overlap_ok = bool(torch.equal(graphs[0].static_output, alone))
            if not overlap_ok:
                raise SystemExit("bench.py: a graph replayed among %d others differs from the same graph replayed alone" % (P - 1))
            out = graphs[0].static_output
        # instrumented eager region (same K steps) for the per-kernel figures
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        with ops.kernel_timing() as rec:
            t1 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            eager_ms = (time.perf_counter() - t1) * 1e3 / args.steps
        rec_store = None
        index_max_alone_ms = None
        if ops.FUSE_POOL:
            ops.FUSE_POOL = False
            try:
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                with ops.kernel_timing() as rec_store:
                    for _ in range(3):
                        step()
                    torch.cuda.synchronize()
                # ... and the pool ALONE on the tensor the last of those steps stored (the in-step launch above reads 1.47 GB the kernel
                # before it has just written; this one finds the tensor at rest): same launch, same bytes
                try:
                    y_st, ids_st = enc.first_pn_out, enc._lazy["a"].min_idx_i32
                    if y_st is not None and y_st.dtype == torch.float32:
                        for _ in range(3):
                            ops.index_max_gather(y_st, ids_st, inp["node"].shape[2], None)
                        e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0_.record()
                        for _ in range(10):
                            ops.index_max_gather(y_st, ids_st, inp["node"].shape[2], None)
                        e1_.record()
                        torch.cuda.synchronize()
                        index_max_alone_ms = e0_.elapsed_time(e1_) / 10
                    del y_st, ids_st
                except Exception:                                  # noqa: BLE001 -- an extra figure, never the reason for a missing line
                    index_max_alone_ms = None
            finally:
                ops.FUSE_POOL = True
        # the replayed forward's operand-range log (fp16-split arithmetic): a violation would mean clamped features
        # (the graphs of a device share its range log: graph 0 is replayed alone right before the log is read)
        if use_graph:
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                graphs[0](inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])
            torch.cuda.synchronize()
        range_bad = graphed.range_violations() if use_graph else []
        if range_bad:
            raise SystemExit("bench.py: h3 operand range violated on the synthetic batch: %s" % (range_bad[:3],))
        # the other two arithmetics of the same path on the same batch (graph replay, same K): extra keys, not `value`
        other = {}

        def measure_other_arithmetics():
            # (called AFTER the BASELINE configs of `other_configs`: extra keys, and ten seconds of matrix-heavy forwards in front of the training
            #  entries would only warm the chip up for them)
            if not (world == 1 and not args.no_other_precisions and use_graph):
                return
            from sonet_hip.graph import GraphedForward
            for mode in ("bf16", "x3", "f32"):
                if mode == ops.POINTMLP_PRECISION:
                    continue
                with ops.precision(mode):
                    g2 = GraphedForward(lambda pc, sn, node, knn: cls(enc(pc, sn, node, knn, is_train=False)),
                                        (inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"]), warmup=2)
                    for _ in range(3):
                        g2(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    for _ in range(args.steps):
                        g2(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t2
                other[mode] = {"clouds_per_s": round(B * args.steps / dt, 1), "ms_per_step": round(dt * 1e3 / args.steps, 4), "in_flight": 1}
                del g2
    line = headline(args, world, rank, dev, elapsed, window_s, P, use_graph, spin_calls, host_pin)

    train_entries = None
    if world > 1 and not args.no_other_configs:
        # BASELINE configs[4] on the driver's multi-GPU command: every rank takes part (gradient all-reduce), rank 0 keeps the entries
        if use_graph:
            del graphs, graphed
        torch.cuda.empty_cache()
        train_entries = other_configs(args, dev, world, rank)
    if rank != 0:
        return

    def kernel_entries(summary, steps, suffix=""):
        out = []
        for name, s_ in sorted(summary.items(), key=lambda kv: -kv[1]["total_ms"]):
            bound, amount = algorithmic(name, B, N)
            k = {"name": name + suffix, "launches_per_step": s_["count"] // steps, "mean_ms": round(s_["mean_ms"], 5),
                 "ms_per_step": round(s_["total_ms"] / steps, 5), "bound": bound}
            if amount:
                if bound == "mfma":
                    ach = amount / (s_["mean_ms"] * 1e-3) / 1e12
                    peak = (PEAK_H3_TFLOPS if name.startswith(("pointresnet_fused", "pointmlph3", "pointmlpws")) else PEAK_X3_TFLOPS if name.startswith("pointmlpx3")
                            else PEAK_BF16_MFMA_TFLOPS if name.startswith(("pointresnet_bf16", "pointmlpbf16")) else PEAK_F32_MFMA_TFLOPS)
                    k.update(achieved=round(ach, 3), peak=round(peak, 1), unit="TFLOP/s", frac=round(ach / peak, 4))
                else:
                    ach = amount / (s_["mean_ms"] * 1e-3) / 1e9
                    k.update(achieved=round(ach, 1), peak=PEAK_HBM_GBS, unit="GB/s", frac=round(ach / PEAK_HBM_GBS, 4))
                    if name.startswith("som_assign"):          # (som_assign_sort: the two launches together, distance arithmetic only)
                        # 64 nodes per 12-byte point: 13 VALU operations per node-point pair (8 for the exact, un-contracted
                        # distance, 1 to pack the key, 4 for the 4-deep min / median chain) put this kernel on the vector-issue
                        # roof long before the HBM one -- at B = 64 (320 k points, ~15 us of arithmetic) it is launch- and
                        # atomics-bound, the vector roof shows at larger batches (tools/microbench.py som)
                        lane_ops = 13.0 * B * N * 64
                        k["valu"] = {"achieved": round(lane_ops / (s_["mean_ms"] * 1e-3) / 1e12, 2), "peak": PEAK_VALU_TLANEOPS,
                                     "unit": "T lane-ops/s", "frac": round(lane_ops / (s_["mean_ms"] * 1e-3) / 1e12 / PEAK_VALU_TLANEOPS, 4)}
            out.append(k)
        return out

    kernels = kernel_entries(rec.summary(), args.steps)
    # The training / segmenter data path keeps first_pn_out (store variant of the fused kernel + index_max_gather + som_group):
    # same inputs, a few instrumented steps, so that the segmented arg-max pool has its roofline line here as well.
    store_path = []
    if rec_store is not None:
        store_path = [k for k in kernel_entries(rec_store.summary(), 3, " [store path]")
                      if k["name"].startswith(("index_max", "pointresnet_fused_L", "som_group"))]
        for k in store_path:
            if k["name"].startswith("index_max") and index_max_alone_ms and "achieved" in k:
                gbs = k["achieved"] * k["mean_ms"] / index_max_alone_ms
                k["standalone"] = {"mean_ms": round(index_max_alone_ms, 5), "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                   "frac": round(gbs / PEAK_HBM_GBS, 4),
                                   "what": "the same launch repeated on the stored tensor at rest (10 calls, HIP events); the in-step figure is taken right "
                                           "behind the kernel that wrote its 1.47 GB input"}
    traffic = {}
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")      # HBM bytes per launch from rocprofv3 --pmc passes
    if os.path.exists(tpath):
        try:
            allt = json.load(open(tpath))
            traffic = dict(allt.get("B%d_N%d" % (B, N), {}))
            if ops.POINTMLP_PRECISION == "bf16":
                traffic.update(allt.get("B%d_N%d_bf16" % (B, N), {}))
        except Exception:
            traffic = {}
    for k in kernels:
        if k["name"] in traffic:
            k["traffic"] = traffic[k["name"]]
            k["traffic_source"] = "profiles/pmc_traffic.json (rocprofv3 --pmc passes of an earlier run of this command; not measured in this run)"
    dom = next((k for k in kernels if "achieved" in k), None)
    roofline = None
    if dom is not None:
        roofline = {"kernel": dom["name"], "bound": dom["bound"], "achieved": dom["achieved"], "peak": dom["peak"],
                    "unit": dom["unit"], "frac": dom["frac"], "mean_ms": dom["mean_ms"], "traffic": dom.get("traffic"),
                    "traffic_source": dom.get("traffic_source")}
        if dom["bound"] == "mfma" and rank == 0 and ops.POINTMLP_PRECISION == "h3":
            # `peak` is the nominal dense rate (2.4 GHz).  With all 256 CUs on the matrix pipe the chip is power-limited:
            # a pure fp16 MFMA loop on operands with random mantissas holds well under that (finding 8).
            # Measured here, on this device, outside the timed region, and quoted in the same algorithmic unit (/3).
            try:
                tf, ghz = ops.mfma_f16_sustained_rate(random_operands=True, iters=4000)
                roofline["sustained"] = {"what": "pure v_mfma_f32_32x32x16_f16 loop, random fp16 operands, all CUs, measured in this run",
                                         "mfma_tflops": round(tf, 1), "shader_ghz": round(ghz, 3), "peak": round(tf / 3.0, 1),
                                         "frac": round(dom["achieved"] / (tf / 3.0), 4)}
            except Exception as e:  # the probe is a diagnostic: never fail the bench on it
                roofline["sustained"] = {"error": str(e)}
    line.update({
        "single_stream": single, "replay_among_others_equals_replay_alone": overlap_ok, "other_arithmetics": other,
        "range_guard": {"enabled": bool(ops.RANGE_GUARD), "violations": len(range_bad)},
        "eager_instrumented_ms_per_step": round(eager_ms, 4),
        "roofline": roofline,
        "kernel_ms_per_step": round(sum(k["ms_per_step"] for k in kernels), 4),
        "kernels": kernels,
        "kernels_store_path": store_path,
    })
    if not args.no_parity_check:
        line["parity_checked"] = parity_check(args, enc, cls, inp, out, enc_cpu, cls_cpu)
    if world == 1 and not args.no_other_configs:
        if use_graph:
            del graphs, graphed
        torch.cuda.empty_cache()
        line["other_configs"] = other_configs(args, dev, 1, 0)
    elif train_entries:
        line["other_configs"] = train_entries
    measure_other_arithmetics()                                # (fills line["other_arithmetics"]: the same dict object)
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(args, enc_cpu, cls_cpu)
    line["summary"] = _summary(line, B, N, world)             # LAST key: a record that keeps only the tail of the line keeps this
    return line


def _summary(line, B, N, world):
    """The figures a reader of the line wants first, in under 2000 characters and at the very END of the JSON line (the driver's
    record keeps the last 2000 characters).  Everything here is a copy of, or simple arithmetic on, entries further up the line."""
    ms = line["ms_per_step"]
    roof = line.get("roofline") or {}
    out = {"value": line["value"], "value_median": line["value_median"], "ms_per_step": ms,
           "windows_clouds_per_s": line["windows"]["clouds_per_s"],
           "single_stream": (line.get("single_stream") or {}).get("clouds_per_s")}
    if roof.get("bound") == "mfma":
        # the whole forward as ONE roofline figure: SURVEY 8(a) totals 5.6 GFLOP per cloud (first PointNet 4.927 + KNNModule 0.53 + final
        # PointNet 0.15); `value` in clouds/s x that = useful TFLOP/s of the step, against the same ceilings as the dominant kernel
        step_tf = line["value"] / world * 5.6e9 / 1e12
        sus = (roof.get("sustained") or {}).get("peak")
        out["step"] = {"useful_tflops": round(step_tf, 1), "frac_of_nominal": round(step_tf / roof["peak"], 4),
                       "frac_of_sustained": round(step_tf / sus, 4) if sus else None,
                       "what": "5.6 GFLOP per cloud x clouds/s: the time outside the fused kernel is matrix work of the node-level stage at "
                               "about the same rate, not idle time (DESIGN.md section 9)"}
        out["fused_kernel"] = {"mean_ms": roof.get("mean_ms", None), "frac": roof["frac"], "frac_of_sustained": (roof.get("sustained") or {}).get("frac")}
    som = [k for k in line.get("kernels", []) if k["name"].startswith("som_assign")]
    if som:
        k = som[0]
        t = k.get("traffic")
        survey_bytes = (121280 + 300768) * B                  # som_assign 121,280 B + som_group 300,768 B per cloud
        out["som_stage"] = {"ms_per_step": k["ms_per_step"], "hbm_frac": k.get("frac"),
                            "hbm_frac_on_survey_8d_bytes": round(survey_bytes / (k["mean_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                            "valu_frac": (k.get("valu") or {}).get("frac"),
                            "pmc_over_algorithmic_bytes": round(t / (k["achieved"] * 1e9 * k["mean_ms"] * 1e-3), 2) if t and k.get("achieved") else None,
                            "pmc_over_survey_8d_bytes": round(t / survey_bytes, 2) if t else None,
                            "bound": "launch latency at this size: 60 % of 8 TB/s would be 5.6 us for both launches (SURVEY 8(d) bytes), below "
                                     "the ~10 us a launch pair costs; neither roof is near (about 2.4 waves per SIMD)"}
    for k in line.get("kernels_store_path", []):
        if k["name"].startswith("index_max"):
            out["index_max"] = {"in_step_frac_of_hbm": k.get("frac"), "standalone_frac_of_hbm": (k.get("standalone") or {}).get("frac")}
    oc = line.get("other_configs") or {}
    out["other_configs"] = {name: ({"ms_per_step": v.get("ms_per_step"), "clouds_per_s": v.get("clouds_per_s"),
                                    "parity_ok": (v.get("parity_checked") or {}).get("ok")} if isinstance(v, dict) else None)
                            for name, v in oc.items()}
    pc = line.get("parity_checked") or {}
    out["parity"] = {"ok": pc.get("ok"), "min_idx_bit_exact": pc.get("min_idx_bit_exact"), "feature_err_over_bound": pc.get("feature_err_over_bound")}
    cb = line.get("cpu_baseline") or {}
    out["cpu_baseline"] = {"clouds_per_s": cb.get("value"), "cores": cb.get("cores"), "kind": cb.get("kind")}
    return out


if __name__ == "__main__":
    _line = None
    try:
        _line = main()
    finally:
        from sonet_hip import dp as _dp
        _dp.shutdown()                     # (RCCL prints its banner on stdout: leave the group first, the JSON line goes LAST)
    if _line is not None:
        import ctypes
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)     # RCCL's banner sits in the C stdio buffer of a piped stdout: out with it first
        print(json.dumps(_line), flush=True)
