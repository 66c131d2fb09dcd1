"""MPPI solve benchmark (BASELINE.json metric: trajectory-steps/sec (K x H per solve) + wall-clock per solve).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload humanoid_ca|cartpole|humanoid_mlp|quad_mlp|cartpole_fa|quad_fa]
                    [--full] [--dump-outputs DIR]

A plain run sets up, ramps the clock, warms up, times the K steps and prints the result line (the rollout's roofline
figures come from device-clock stamps inside the timed region).  --full adds the measurements that take runs of their
own: the rocprofv3 kernel-trace and PMC traffic child passes, the HIP-event pass over plain solves and the CPU
baseline (each can be left out again with its --no-... option).  --dump-outputs DIR writes the controls the last
timed step left (DIR/U.npy, DIR/u0.npy, streams also DIR/x0.npy; float32): the warmup and timed steps start from a
fixed state, so two runs with the same arguments write the same arrays.
One step = one batched MPPI solve per rank (noise -> rollout -> cost -> softmin -> reduce -> update -> shift),
replayed from a captured hipGraph with inputs resident in HBM, then (N > 1) an RCCL all-gather of the reduced
control sequences U* and u0 (overlapped with the next step's solve; all gathers complete inside the timed region).  Stream workloads chain 256 solves (with the on-device env step) per step.
Default workload = BASELINE config #4 as BASELINE states it: humanoid CrossAttention surrogate
(checkpoints/model_cross.pth), K=1024, H=64, 64 independent solves (x0 = rows 20*i of
data/2025-04-09_145305/states.csv) sharded across the GPUs (strong scaling: all 64 on one GPU at N=1, 8 per GPU at
N=8, then the RCCL gather of the controls).  --global-solves G splits another total; --weak runs the whole config #4
on every GPU (64 solves per rank, no data-path collective: weak scaling); --solves B sets another per-rank batch (weak).
For N>1 launch with torch.distributed.run.
Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "humanoid_mppi-rl_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

METRIC = "trajectory-steps/sec (K×H per solve) + wall-clock per MPPI solve, 1/2/4/8 GPU"
PEAK_BF16 = 2.5e15  # dense MFMA, MI355X_MICROARCH.md
PEAK_FP32 = 157.3e12
PEAK_HBM = 8.0e12
CA_FLOP_FOLDED = 93_696  # per sample-step, SURVEY 8a a4 (folded cross-attention)
MLP_FLOP = lambda nx, nu, h=128: 2 * ((nx + nu) * h + 2 * h * h + h * nx)  # noqa: E731


# The arithmetic each workload runs by default.  Config #4 (humanoid, K=1024 H=64) is quoted at the reference's own
# precision: the reference evaluates the CA net in fp32 torch (src/cartpole_mppi_estimator.py:89-93, learning/model.py:
# 157-202) and the humanoid loop in fp64 (src/Humanoid_mppi_v3.jl:128-170), and BASELINE grants it no bf16, so it runs
# the fp32-accurate split mode (costs within rtol 1e-4 of the fp32 oracle, tests/test_gpu_fullsize.py).  Configs #3
# (quadruped, "bf16 rollouts / fp32 reduce") and #5 (humanoid stream, "bf16") are bf16 as BASELINE.json states them.
DEFAULT_PRECISION = {"humanoid_ca": "bf16x3", "humanoid_mlp": "bf16x3", "humanoid_ca_stream": "bf16",
                     "quad_mlp": "bf16", "quad_fa": "bf16", "cartpole_fa": "bf16", "cartpole": "fp32"}


def fa_flop(L: int, D: int, layers: int = 2) -> int:
    """FeatureAttentionStatePredictor FLOP per sample-step: per layer 24 L D^2 (q,k,v, out-proj, FFN)
    + 4 L^2 D (scores, P V); encoding + output layer 2 L D each."""
    return layers * (24 * L * D * D + 4 * L * L * D) + 4 * L * D


def workload_spec(name: str, precision: str, solves: int = 0, global_solves: int = 64, world: int = 1):
    """The humanoid batched workloads are BASELINE config #4: 64 independent solves (64 initial states) split over the
    ranks by default (global_solves = 64: strong scaling, 8 per GPU at N = 8); solves > 0 instead sets a per-rank batch
    (weak scaling: bench.py --weak = 64 per rank, the whole config #4 on every GPU)."""
    import mppi_hip
    prec = {"bf16": 1, "fp32": 0, "bf16x3": 2}[precision]
    G = 0 if solves or name not in ("humanoid_ca", "humanoid_mlp") else global_solves
    # strong scaling over a world that does not divide G: contiguous shards of ceil(G / world) (the last ranks get
    # fewer, mppi_hip.distributed.shard_bounds); every rank sizes its buffers (and the gather) for ceil(G / world)
    Bh = solves or (-(-G // world) if G else 64)
    gold = os.path.join(REPO, "tests", "golden")
    if name == "humanoid_ca":
        sd = mppi_hip.load_npz(os.path.join(gold, "ca_humanoid_weights.npz"))
        x0_all = np.load(os.path.join(gold, "g5_ca_humanoid_fwd.npz"))["x0_stride20"]
        cfg = mppi_hip.Config.preset("humanoid_v3", K=1024, H=64, precision=prec, max_batch=Bh)
        return dict(cfg=cfg, dyn=mppi_hip.cross_attention_blob(sd), cost="humanoid_v3", B=Bh, x0_all=x0_all,
                    flop=CA_FLOP_FOLDED, bound="mfma", sd=sd, global_solves=G,
                    desc="humanoid CrossAttention surrogate (checkpoints/model_cross.pth, folded), cost "
                         f"Humanoid_mppi_v3.jl, K=1024 H=64, {Bh} solves/GPU (BASELINE config #4: 64 states)")
    if name == "humanoid_ca_stream":
        sd = mppi_hip.load_npz(os.path.join(gold, "ca_humanoid_weights.npz"))
        x0_all = np.load(os.path.join(gold, "g5_ca_humanoid_fwd.npz"))["x0_stride20"]
        cfg = mppi_hip.Config.preset("humanoid_v3", K=8192, H=128, precision=prec, max_batch=1)
        return dict(cfg=cfg, dyn=mppi_hip.cross_attention_blob(sd), cost="humanoid_v3", B=1, x0_all=x0_all,
                    flop=CA_FLOP_FOLDED, bound="mfma", sd=sd, stream=256,
                    desc="humanoid CrossAttention surrogate, K=8192 H=128, receding-horizon stream of 256 solves/GPU "
                         "(shift + on-device env step) replayed as one hipGraph per step (BASELINE config #5)")
    if name == "humanoid_mlp":
        sd = mppi_hip.synthetic_mlp(55, 21, seed=0)
        x0_all = np.load(os.path.join(gold, "g5_ca_humanoid_fwd.npz"))["x0_stride20"]
        cfg = mppi_hip.Config.preset("humanoid_v3", K=1024, H=64, precision=prec, max_batch=Bh)
        return dict(cfg=cfg, dyn=mppi_hip.mlp_blob(sd, 55, 21), cost="humanoid_v3", B=Bh, x0_all=x0_all, sd_mlp=sd,
                    flop=MLP_FLOP(55, 21), bound="mfma", global_solves=G,
                    desc=f"humanoid MLPStatePredictor(55,21,128,2) seeded weights, K=1024 H=64, {Bh} solves/GPU "
                         "(config #4's shape)")
    if name == "quad_mlp":
        # BASELINE config #3: the MLP surrogate trained on the reference's own quadruped logs by mppi_hip.training
        # (learning/train_quadruped.py's recipe; checkpoints_quadruped is missing), x0 = logged states
        sd = {k: v for k, v in mppi_hip.load_npz(os.path.join(gold, "quad_mlp_trained.npz")).items()
              if k.startswith("network.")}
        logs = np.load(os.path.join(gold, "quad_logs.npz"))
        x0_all = np.ascontiguousarray(logs["states0"][2::40][:64], np.float32)
        cfg = mppi_hip.Config.preset("quad_est", K=2048, H=40, precision=prec, max_batch=1)
        return dict(cfg=cfg, dyn=mppi_hip.mlp_blob(sd, 37, 12), cost="quad_est", B=1, x0_all=x0_all, sd_mlp=sd,
                    flop=MLP_FLOP(37, 12), bound="mfma",
                    desc="quadruped MLPStatePredictor(37,12,128,2) trained on the reference's quad_data logs "
                         "(mppi_hip.training), x0 = logged states, K=2048 H=40 (BASELINE config #3)")
    if name == "cartpole_fa":
        sd = mppi_hip.load_npz(os.path.join(gold, "fa_cartpole_weights.npz"))
        x0_all = np.tile(np.array([[0.05, 0.1, 0.0, 0.0]], np.float32), (64, 1))
        cfg = mppi_hip.Config.preset("cartpole_est", precision=prec, max_batch=1)
        return dict(cfg=cfg, dyn=mppi_hip.feature_attention_blob(sd, 4, 1, 64), cost="cartpole_est", B=1,
                    x0_all=x0_all, flop=fa_flop(5, 64), bound="mfma", sd=sd, nx=4, nu=1,
                    desc="cartpole FeatureAttention estimator (checkpoints_cartpole/model_best.pth, hidden 64, 2 layers), "
                         "preset cartpole_est K=2048 H=100 (src/cartpole_mppi_estimator.py:28-40)")
    if name == "quad_fa":
        sd = mppi_hip.synthetic_feature_attention(37, 12, 512, seed=0)
        x0_all = np.zeros((64, 37), np.float32)
        x0_all[:, 2] = 0.35
        x0_all[:, 3] = 1.0
        cfg = mppi_hip.Config.preset("quad_est", K=2048, H=40, precision=prec, max_batch=1)
        return dict(cfg=cfg, dyn=mppi_hip.feature_attention_blob(sd, 37, 12, 512), cost="quad_est", B=1,
                    x0_all=x0_all, flop=fa_flop(49, 512), bound="mfma", sd=sd, nx=37, nu=12,
                    desc="quadruped FeatureAttention estimator (hidden 512, 4 heads, 2 layers, 49 tokens; seeded weights, "
                         "checkpoints_quadruped missing), K=2048 H=40 (config #3 shape, src/quadruped_mppi_estimator.py)")
    if name == "cartpole":
        cfg = mppi_hip.Config.preset("cartpole_py", K=4096, H=50, precision=0, max_batch=1)
        x0_all = np.tile(np.array([[0.0, np.pi, 0.0, 0.0]], np.float32), (64, 1))
        return dict(cfg=cfg, dyn=(1, None), cost="cartpole", B=1, x0_all=x0_all, flop=0, bound="hbm",
                    desc="analytic cartpole (models/cartpole.xml), K=4096 H=50, 1 solve/GPU (BASELINE config #2)")
    raise SystemExit(f"unknown workload {name}")


def workload_kernel(name: str) -> str:
    """The dominant (roofline) kernel of a workload."""
    if name == "cartpole_fa" and os.environ.get("MPPI_FA_SMALL", "1") != "0":
        return "fa_small_kernel"  # the small-net kernel (hidden 64, <= 16 tokens, bf16)
    if name == "quad_fa" and os.environ.get("MPPI_FA_LAYERED", "") == "1":
        return "fal_gemm_kernel"  # the layer-by-layer path (kernels_fa_layered.hip): its GEMMs dominate
    if name in ("cartpole_fa", "quad_fa"):
        return "fa_rollout_kernel"
    return "cartpole_rollout_kernel" if name == "cartpole" else "fc_rollout_kernel"


def cpu_baseline(name: str, spec: dict, threads: int) -> dict:
    """Oracle-side CPU baseline ("port"), timed on this host's cores, bounded to ~10-30 s.

    fc nets and the analytic cartpole: oracle/mppi_cpu.c, the compiled OpenMP restatement of the solve (the
    counterpart of the reference's threaded Julia rollout, src/Humanoid_mppi_v3.jl:131), median of 20 full solves
    after 3 warm-ups.  The slower torch-CPU / serial-Python ports of the reference's own loop shapes are
    timed beside it and quoted in `sample`.  FA nets: the torch-CPU port only."""
    cfg = spec["cfg"]
    if name in ("humanoid_ca", "humanoid_ca_stream", "humanoid_mlp", "quad_mlp"):
        from oracle import cpu as C
        from oracle import mppi_ref as R
        from oracle import nets_ref as N
        C.build()
        extra = ""
        if name.startswith("humanoid_ca") and cfg.K * cfg.H <= 1024 * 64:  # first: libgomp's spinning threads
            from oracle.torch_port import time_humanoid_baseline        # would slow torch's pool afterwards
            t = time_humanoid_baseline(spec["sd"], spec["x0_all"][0], K=cfg.K, H=cfg.H, threads=threads, budget_s=8.0)
            extra = (f"; beside it the torch-CPU port of src/cartpole_mppi_estimator.py:61-143 with the unfolded net "
                     f"(oracle/torch_port.py): {t['value']:.3g} trajectory-steps/s, {t['ms_per_solve']:.1f} ms/solve")
        if name.startswith("humanoid_ca"):
            stack, net = N.ca_fold(spec["sd"], 28, 27, 21), "CrossAttention net (folded exactly, oracle/nets_ref.py:ca_fold)"
        else:
            stack, net = N.mlp_stack(spec["sd_mlp"]), "MLPStatePredictor net"
        ctx = R.humanoid_context() if spec["cost"] == "humanoid_v3" else np.array([2.0, 0.0, 0.35, 0, 0, 0, 0, 0])
        r = C.time_fc_baseline(stack, cfg.nx, cfg.nu, spec["cost"], spec["x0_all"][0], K=cfg.K, H=cfg.H,
                               sigma=cfg.sigma, lam=cfg.lambda_, ctx=ctx, threads=threads,
                               ctrl_clamp=cfg.ctrl_clamp, U_clamp=cfg.U_clamp, norm_eps=cfg.norm_eps,
                               terminal_weight=cfg.terminal_weight, replace=cfg.update_mode != 0)
        return dict(value=r["value"], unit="trajectory-steps/s", cores=threads, kind="port",
                    sample=f"median of {r['solves']} full solves K={cfg.K} H={cfg.H} (1 x0) after 3 warm-ups: "
                           f"oracle/mppi_cpu.c (C, OpenMP over {threads} threads, fp32, AVX2) with the {net}; "
                           f"{r['ms_per_solve']:.1f} ms/solve{extra}")
    if name in ("cartpole_fa", "quad_fa"):
        from oracle.torch_port import time_fa_baseline
        # quad: one full H=40 solve takes minutes on the host; time a bounded sample of 2 horizon steps
        K, H = cfg.K, (cfg.H if name == "cartpole_fa" else 2)
        r = time_fa_baseline(spec["sd"], spec["x0_all"][0], spec["nx"], spec["nu"], K=K, H=H, cost=spec["cost"],
                             sigma=cfg.sigma, threads=threads, budget_s=20.0)
        return dict(value=r["value"], unit="trajectory-steps/s", cores=threads, kind="port",
                    sample=f"{r['solves']} solves K={K} H={H}, torch-CPU port of src/*_mppi_estimator.py rollouts with "
                           f"nn.MultiheadAttention FA net; median {r['ms_per_solve']:.1f} ms/solve")
    if name == "cartpole":
        from oracle import cartpole_serial as S
        from oracle import cpu as C
        from oracle import mppi_ref as R
        C.build()
        x0 = np.array([0.0, np.pi, 0.0, 0.0])
        r = C.time_cartpole_baseline(x0, K=cfg.K, H=cfg.H, threads=threads)
        # the reference's own loop shape: serial per-sample Python (src/cartpole_mppi.py:59-98), 512 samples
        Ks = 512
        noise = R.reference_noise(0, 1, cfg.H, Ks, 1.0)
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 4.0:
            S.mppi_step(x0, np.zeros((1, cfg.H)), noise)
            n += 1
        dt = (time.perf_counter() - t0) / n
        return dict(value=r["value"], unit="trajectory-steps/s", cores=threads, kind="port",
                    sample=f"median of {r['solves']} full solves K={cfg.K} H={cfg.H} after 3 warm-ups: "
                           f"oracle/mppi_cpu.c (C, OpenMP over {threads} threads, fp64 analytic mj_step); "
                           f"{r['ms_per_solve']:.2f} ms/solve; beside it the serial per-sample Python loop of "
                           f"src/cartpole_mppi.py:59-98 (oracle/cartpole_serial.py, 1 core, K={Ks}): "
                           f"{Ks * cfg.H / dt:.3g} trajectory-steps/s")
    return None


# FETCH_SIZE -> bytes per kernel access pattern (MI355X_MICROARCH.md §HBM: x2 for wide 16-B-per-lane coalesced
# streaming reads; other widths must be calibrated on a known byte count of the kernel's own pattern).  Round 5: both
# eps patterns below calibrated independently of the kernels, on a buffer of exactly config #4's eps read once in the
# kernels' own load pattern (tools/fetch_calib.hip, profiles/r05_fetch_calib.txt): 4-B lane loads in 128-B segments
# (the per-wave kernels) x2.000, in 64-B segments (the M-split kernel) x1.000, 16-B streaming loads x2.000.
#   fc_rollout_kernel: 4-B lane loads of eps at the cost flush (64-B segments); its one known bulk read is eps,
#     once: the raw counter (44.8 MB per config #4 launch) equals those 44.0 MB (+ U, x0, weights), so factor 1.
#   fc_wave_kernel (the per-wave CA kernel, chosen for >= 6 tiles per CU): the same 4-B lane loads, but a wave's two
#     16-sample tiles are adjacent, so each (u, t) row is read as 128 contiguous bytes by two loads; calibrated the same
#     way: raw FETCH_SIZE 178.5 MB per 64-solve launch against its one bulk read, 352.3 MB of eps: factor 2.
#   fa_rollout_kernel: 16-B fragment loads (the guide's calibrated pattern), factor 2.
#   fc_wave_mlp_kernel (the per-wave MLP kernel): the same adjacent-tile eps pattern (8 control slots per lane group),
#     factor 2 as fc_wave_kernel.
#   fc_wave32_kernel (its 32x32x16 variant): a wave's 32 samples are one 128-B load per (u, t) row, factor 2;
#     fc_wave32_x3_kernel and fc_wave32_x3p_kernel (split bf16, per wave) read eps the same way.
#   fc_wave_mlp_x3_kernel (the split per-wave MLP kernel, round 5): one 16-sample tile per wave, so each (u, t) row
#     is read as 64-B segments, the M-split pattern: factor 1.  fc_wave32_mlp_x3_kernel (its 32-sample form): 128-B
#     rows as fc_wave32_kernel, factor 2.
FETCH_FACTOR = {"fc_rollout_kernel": 1.0, "fc_pipe_kernel": 1.0, "fc_wave_kernel": 2.0, "fc_wave_mlp_kernel": 2.0,
                "fc_wave32_kernel": 2.0, "fc_wave32_x3_kernel": 2.0, "fc_wave32_x3p_kernel": 2.0,
                "fc_wave_mlp_x3_kernel": 1.0, "fc_wave32_mlp_x3_kernel": 2.0}
# kernels that can run a workload's rollout (the engine picks fc_wave_kernel for batches with >= 6 tiles per CU,
# fc_pipe_kernel when forced)
KERNEL_ALIASES = {"fc_rollout_kernel": ("fc_rollout_kernel", "fc_wave_kernel", "fc_wave32_kernel", "fc_wave32_x3_kernel",
                                         "fc_wave32_x3p_kernel", "fc_wave_mlp_kernel", "fc_wave_mlp_x3_kernel",
                                         "fc_wave32_mlp_x3_kernel", "fc_pipe_kernel")}


def pmc_traffic(args, kernel_substr: str) -> dict | None:
    """HBM bytes per launch of the dominant kernel from rocprofv3 PMC counters, collected live in two separate
    child passes (FETCH_SIZE, WRITE_SIZE), corrected per MI355X_MICROARCH.md §HBM: bytes = (f*FETCH + WRITE)*1024
    with f = 2 for coalesced 16-B streaming reads (gfx950 FETCH_SIZE counts half of them) or the kernel's own
    calibrated factor (FETCH_FACTOR). None if rocprofv3 is unavailable."""
    import csv
    import shutil
    import subprocess
    import tempfile

    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    vals = {}
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        # one rocprofv3 call, one counter per pass (input file: one "pmc:" line per pass).  With several passes the
        # launcher runs the command as a child per pass instead of exec-ing into it.
        inp = os.path.join(d, "counters.txt")
        with open(inp, "w") as fh:
            fh.write("pmc: FETCH_SIZE\npmc: WRITE_SIZE\n")
        out = os.path.join(d, "pmc")
        cmd = [prof, "-i", inp, "-d", out, "-o", "pmc", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--workload", args.workload, "--precision", args.precision, "--steps",
               "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-traffic", "--no-kernel-trace", "--launch", args.launch,
               "--ramp-ms", "0",
               "--stream-solves",
               "4" if args.stream_solves or "stream" in args.workload else "0", "--solves", str(args.solves),
               "--global-solves", str(args.global_solves)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, WORLD_SIZE="1",
                                                                                     RANK="0", LOCAL_RANK="0"))
        except (subprocess.TimeoutExpired, OSError):
            return None
        if r.returncode != 0:
            return None
        files = [os.path.join(root, f) for root, _, fs in os.walk(out) for f in fs
                 if f.endswith("counter_collection.csv")]
        alts = KERNEL_ALIASES.get(kernel_substr, (kernel_substr,))
        rows = [row for f in files for row in csv.DictReader(open(f))
                if any(k in row["Kernel_Name"] for k in alts)]
        # the solve's rollout launches only: the largest grid (stream workloads also launch the rollout kernel
        # over one sample for the env step)
        gkey = next((k for k in ("Grid_Size", "Grid_Size_X", "Grid_SizeX") if rows and k in rows[0]), None)
        if gkey:
            gmax = max(int(float(r[gkey])) for r in rows)
            rows = [r for r in rows if int(float(r[gkey])) == gmax]
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            xs = [float(row["Counter_Value"]) for row in rows if row["Counter_Name"] == ctr]
            if not xs:
                return None
            vals[ctr] = sum(xs) / len(xs)
        ran = next((k for k in alts if rows and k in rows[0]["Kernel_Name"]), kernel_substr)  # the kernel that ran
    f = FETCH_FACTOR.get(ran, 2.0)
    return dict(bytes=(f * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, fetch_kb=vals["FETCH_SIZE"], factor=f,
                write_kb=vals["WRITE_SIZE"], kernel=ran)


def kernel_trace(args) -> dict | None:
    """Average duration (ms) per launch of every kernel of the timed path: a rocprofv3 --kernel-trace child pass of
    this command with the plain-solve event pass off, so only the timed path's launches (graph replays or chained
    solves) and a few one-off setup kernels run; kernels launched fewer times than the pass has steps are dropped.  Keyed by kernel (with its template arguments: reduce_kernel<true, false> is the graph path's generating
    reduce) and grid (stream workloads also launch the rollout kernel for the one-sample env step)."""
    import csv
    import shutil
    import subprocess
    import tempfile

    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        cmd = [prof, "--kernel-trace", "-d", d, "-o", "kt", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--workload", args.workload, "--precision", args.precision, "--steps", "5",
               "--warmup", "1", "--no-cpu-baseline", "--no-traffic", "--no-kernel-trace", "--no-plain-pass",
               "--launch", args.launch, "--ramp-ms", str(args.ramp_ms),
               "--stream-solves", "4" if args.stream_solves or "stream" in args.workload else "0",
               "--solves", str(args.solves), "--global-solves", str(args.global_solves)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240,
                               env=dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
        except (subprocess.TimeoutExpired, OSError):
            return None
        if r.returncode != 0:
            return None
        files = [os.path.join(root, f) for root, _, fs in os.walk(d) for f in fs if f.endswith("kernel_trace.csv")]
        runs = {}  # (kernel, grid) -> [(start, ns)]: the env step reuses the rollout kernel on a tiny grid
        for f in files:
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("mppi::", "").strip()
                grid = "x".join(row[c] for c in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if c in row)
                runs.setdefault((name, grid or row.get("Grid_Size", "?")), []).append(
                    (float(row["Start_Timestamp"]), float(row["End_Timestamp"]) - float(row["Start_Timestamp"])))
        # the pass ramps the clock like the bench, then runs 6 steps (1 warmup + 5): each kernel of the timed path
        # is averaged over its last 6 steps' launches; one-off setup launches (the runtime's copies and fills at
        # handle creation, the first solve's noise, the seed-counter reset) are left out
        setup = ("__amd_rocclr", "at::native")
        per_step = 4 if args.stream_solves or "stream" in args.workload else 1  # the pass's --stream-solves
        out = {}
        for (n, g), rs in sorted(runs.items()):
            if len(rs) < 5 or n.startswith(setup):
                continue
            last = sorted(rs)[-6 * per_step:]
            out[f"{n} [grid {g}, last {len(last)} of {len(rs)} launches]"] = sum(d for _, d in last) / len(last) * 1e-6
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="humanoid_ca")
    ap.add_argument("--precision", default="auto", choices=["auto", "bf16", "fp32", "bf16x3"],
                    help="arithmetic of the learned-dynamics rollouts (the analytic cartpole always runs fp32); "
                         "bf16x3 = fp32-accurate split (hi + lo pairs, 3 MFMAs per product; fc nets); auto = the "
                         "reference's arithmetic class per workload (DEFAULT_PRECISION)")
    ap.add_argument("--global-solves", type=int, default=64,
                    help="independent solves split over all ranks, humanoid batched workloads (strong scaling; default "
                         "64 = BASELINE config #4's 64 states: all on one GPU at N=1, 8 per GPU at N=8)")
    ap.add_argument("--solves", type=int, default=0,
                    help="independent solves PER RANK instead (weak scaling: every rank its own batch)")
    ap.add_argument("--weak", action="store_true",
                    help="weak scaling: the whole config #4 (64 solves) on every rank, no data-path collective "
                         "(= --solves 64)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the rocprofv3 kernel-trace and PMC traffic "
                         "child passes (kernel_ms, roofline.traffic), the HIP-event pass over plain solves "
                         "(plain_solve_kernel_ms) and the CPU baseline (cpu_baseline); off by default, and each part can "
                         "be left out again with its --no-... option")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the controls the last timed step left, as a caller of the step "
                         "receives them: DIR/U.npy [solves, nu, H] and DIR/u0.npy [solves, nu] (every rank's rows at "
                         "N > 1, from the gather), stream workloads also DIR/x0.npy (the state the stream reached); "
                         "float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-traffic", action="store_true",
                    help="with --full: skip the rocprofv3 PMC passes for roofline.traffic")
    ap.add_argument("--stream-solves", type=int, default=0, help="override the stream length (stream workloads)")
    ap.add_argument("--no-kernel-trace", action="store_true",
                    help="with --full: skip the rocprofv3 kernel-trace pass that times the graph path's kernels "
                         "(kernel_ms)")
    ap.add_argument("--no-plain-pass", action="store_true",
                    help="with --full: skip the HIP-event pass over plain solves before the timed region")
    ap.add_argument("--ramp-ms", type=float, default=150.0,
                    help="untimed GPU work (the same steps) before the warmup steps, so the timed region runs at "
                         "steady-state clocks: after an idle host phase the GPU clock ramps over ~20 ms of load "
                         "(config #4: 113 us/step timed right after 5 warmup steps, 104.5 us at steady state)")
    ap.add_argument("--gather-every", type=int, default=4,
                    help="steps per control all-gather at N > 1: each step's U*, u0 are snapshotted at that step and "
                         "m steps' snapshots leave in one RCCL collective (a collective costs ~6 us of GPU time beside "
                         "the solves even at world 1: scripts/gather_probe.py)")
    ap.add_argument("--launch", choices=["auto", "graph", "chain"], default="auto",
                    help="how a step is launched: graph replay, or chained stream launches (MPPI_FLAG_CHAIN); auto = "
                         "graph for the receding-horizon streams (256 solves per launch), chain for one solve per step")
    args = ap.parse_args()
    if args.precision == "auto":
        args.precision = DEFAULT_PRECISION.get(args.workload, "bf16")
    if args.weak and not args.solves:
        args.solves = 64
    if not args.full:  # a plain run: only what the headline figure needs
        args.no_cpu_baseline = args.no_traffic = args.no_kernel_trace = args.no_plain_pass = True

    # --gpus N is the number of ranks: without a launcher start N ranks under torch.distributed.run (before any GPU
    # call in this process), under one it must agree with WORLD_SIZE
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # rocprofv3 child passes (graph-path kernel trace, PMC traffic) run FIRST, before this process touches the GPU:
    # the profiler's launcher replaces itself (exec) with the profiled command, which the GPU pool forbids in any
    # process descending from one that has initialised the GPU
    ktr = tr = None
    if world == 1:
        if not args.no_kernel_trace:
            ktr = kernel_trace(args)
        if not args.no_traffic:
            tr = pmc_traffic(args, workload_kernel(args.workload))

    import torch
    import torch.distributed as dist

    local = int(os.environ.get("LOCAL_RANK", "0"))
    # one process per GPU (RCCL = "nccl" backend). MPPI_DIST_BACKEND=gloo + ranks sharing device 0 rehearses the
    # multi-rank path on a single-GPU box; the driver's N-GPU runs use the default.
    backend = os.environ.get("MPPI_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    # MPPI_FORCE_GATHER=1 runs the RCCL gather path at world 1 (one-GPU box: measures its host overhead per step)
    force_gather = os.environ.get("MPPI_FORCE_GATHER") == "1"
    if force_gather and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or force_gather:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import mppi_hip
    spec = workload_spec(args.workload, args.precision, args.solves, args.global_solves, world)
    cfg = spec["cfg"]
    Bmax = spec["B"]  # this rank's buffer rows (the gathered shard size)
    from mppi_hip.distributed import shard_bounds
    G = spec.get("global_solves") or world * Bmax
    start, stop, _ = shard_bounds(G, rank, world)
    B = stop - start  # the solves this rank runs (uneven strong shards: the last ranks may run fewer)
    if B < 1:
        raise SystemExit(f"bench.py: {G} global solves leave rank {rank} of {world} without a solve")
    eng = mppi_hip.Engine(cfg, device=dev.index)
    eng.load_dynamics(*spec["dyn"]).set_cost(spec["cost"])
    stream = torch.cuda.current_stream(dev)
    eng.set_stream(stream.cuda_stream)

    # this rank's shard of the initial states (independent solves; no data-path collective). Weak scaling:
    # B solves per rank; the global list is rows 0..G-1 of the x0 table (config #4: 64 rows over 8 ranks).
    rows = np.arange(start, stop) % spec["x0_all"].shape[0]
    x0 = torch.from_numpy(np.ascontiguousarray(spec["x0_all"][rows], np.float32)).to(dev)
    x0_init = x0.clone()
    # nominal sequences U [B, nu, H] (resident in HBM, updated in place) and u0 [B, nu]: views of one flat buffer,
    # so each step's controls leave the rank with one snapshot copy and ONE all-gather
    from mppi_hip.distributed import control_buffers
    flat_ctrl, U, u0 = control_buffers(Bmax, cfg.nu, cfg.H, device=dev)

    n_stream = args.stream_solves or spec.get("stream", 0)
    env_step = n_stream > 0  # the receding-horizon stream advances x0 on device between its solves
    # Plain-solve kernel durations: HIP events around each launch of 16 plain solves (noise_kernel -> rollout ->
    # block-local reduce) before the timed region, reported as plain_solve_kernel_ms.  The timed region replays the
    # graph path instead (rollout -> reduce_kernel<GEN>, no noise launch): its rollout launches are timed on the
    # device clock inside the timed region (below) and all its kernels by the rocprofv3 kernel-trace pass.
    prof_kt = None
    if not args.no_plain_pass:
        for i in range(20):
            if i == 4:  # 4 warm-up solves, then 16 profiled
                torch.cuda.synchronize(dev)
                eng.profile(True)
            eng.solve_device(B, x0.data_ptr(), U.data_ptr(), None, seed=rank << 40, u0_ptr=u0.data_ptr(), shift=True,
                             env_step=env_step, seed_counter=True)
        torch.cuda.synchronize(dev)
        eng.profile(False)
        prof_kt = {k: eng.kernel_time(k) for k in ("noise", "rollout", "reduce")}
    # One step = max(n_stream, 1) solves (rollout -> reduce_kernel<GEN>, which also generates the next solve's noise
    # [-> env step]); the device seed counter gives every solve fresh noise.  Streams replay a captured hipGraph (one
    # launch per 256 solves); one solve per step is chained on the stream (MPPI_FLAG_CHAIN, the same two kernels):
    # a graph launch pays a fixed ~8.5 us gap at its boundary that back-to-back stream launches do not (rocprof trace,
    # DESIGN.md §5).  Rollout launches are timed on the device clock (mppi_kernel_clock, no event in the stream).
    launch = args.launch if args.launch != "auto" else ("graph" if n_stream > 0 else "chain")
    eng.kernel_clock(True)
    if launch == "graph":
        eng.graph_capture(B, max(n_stream, 1), x0.data_ptr(), U.data_ptr(), u0.data_ptr(), seed=rank << 40,
                          env_step=env_step)

    # RCCL over xGMI gathers only the reduced control sequences. Pipelined: step i's U*, u0 are
    # snapshotted on the compute stream at step i (the next solve updates U in place) and gathered on RCCL's stream,
    # --gather-every steps' snapshots per collective, while the following steps solve; every gather is complete
    # (drain) inside the timed region.
    from mppi_hip.distributed import ControlGatherer
    gather = ControlGatherer(U, u0, flat=flat_ctrl, every=args.gather_every) if (world > 1 or force_gather) else None
    # chained solves with the gather: U stays resident in the engine (MPPI_FLAG_RESIDENT_U) and each solve's update
    # kernel also writes the new U (and u0) straight into this step's place in the gather slot: no snapshot copy
    mirror = gather is not None and launch == "chain"
    if mirror:
        eng.set_U(U[:B].cpu().numpy(), B)

    last = [None]  # the gather handle of the newest gathered step (--dump-outputs reads its result)

    def step(i, gathered=True):
        if launch == "graph":
            eng.graph_launch(sync=False)
        elif mirror:
            h, Us, u0s = gather.reserve() if gathered else (None, U, u0)
            eng.solve_device(B, x0.data_ptr(), Us.data_ptr(), None, seed=rank << 40, u0_ptr=u0s.data_ptr(),
                             shift=True, resident_U=True, env_step=env_step, seed_counter=True, chain=True)
            if gathered:
                last[0] = gather.commit()
            return
        else:
            eng.solve_device(B, x0.data_ptr(), U.data_ptr(), None, seed=rank << 40, u0_ptr=u0.data_ptr(), shift=True,
                             env_step=env_step, seed_counter=True, chain=True)
        if gather is not None and gathered:
            last[0] = gather.submit(U, u0)

    # clock ramp: the same steps, untimed, for at least --ramp-ms of wall time, then the W warmup steps.  Each rank
    # times its own ramp, so the ramp steps run without the control gather: a collective per ramp step would pair
    # up different step counts across ranks and deadlock.
    t_ramp, n_ramp = time.perf_counter(), 0
    while (time.perf_counter() - t_ramp) * 1e3 < args.ramp_ms:
        for _ in range(8 if n_stream == 0 else 1):  # a stream step is ~50 ms
            step(-1, gathered=False)
            n_ramp += 1
        torch.cuda.synchronize(dev)
    # a fixed start for the warmup and timed steps: the ramp (and the plain-solve pass) ran a number of solves that
    # differs from run to run, and every solve moves U, the noise key counter and a stream's x0.  Back to the initial
    # states, zero controls and key 0, so the same arguments give the same steps, output for output (--dump-outputs).
    # The reset drops the prefetched noise, so the first step after it generates its own again (a warmup step).
    torch.cuda.synchronize(dev)
    x0.copy_(x0_init)
    flat_ctrl.zero_()
    if mirror:
        eng.set_U(U[:B].cpu().numpy(), B)
    eng.set_seed_counter(0)
    for i in range(args.warmup):
        step(i)
    if gather is not None:
        gather.drain()
    torch.cuda.synchronize(dev)
    eng.kernel_clock(True)  # reset: count only the timed region's rollout launches
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    if gather is not None:
        gather.drain()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    n_roll, us_roll, us_roll_max = eng.kernel_clock_read()  # rollout launches of the timed region
    routed = eng.rollout_kernel()  # the kernel the engine routed the timed solves' rollouts to (mppi_rollout_kernel)
    l1_products, l1_probe = eng.x3_layer1()  # the split CA's layer 1: the engine's probe of these weights
    f16_on, f16_probe = eng.x3_f16()  # ... and fc_wave32_x3p_kernel's fp16 form (mppi_x3_f16)
    # the fp16 form the routed kernel ran: every layer and the statistic ("<f16...>"), or layers 1 and 2 only
    # ("<l1=f16...>", builds with MPPI_X3_F16_L0=0); the last layer as one fp16 product (",l2=1>") or two
    f16_all = bool(f16_on) and "<f16" in routed
    f16_l1 = bool(f16_on) and "<l1=f16" in routed
    f16_l2x1 = (f16_all or f16_l1) and routed.endswith(",l2=1>")
    f16_ran = f16_all or f16_l1

    if args.dump_outputs and rank == 0 and args.steps > 0:
        # what the last timed step handed its caller: the updated (shifted) U and the applied controls u0 -- this
        # rank's own at N = 1, every rank's from that step's gather otherwise (each rank's rows up to its shard's
        # size: the rows behind a short shard are padding) -- and, for a stream, the state its env steps reached
        if gather is not None:
            U_all, u0_all = gather.result(last[0])
            bounds = [shard_bounds(G, r, world) for r in range(world)]
            keep = np.concatenate([r * Bmax + np.arange(stop_r - start_r) for r, (start_r, stop_r, _) in enumerate(bounds)])
            outs = {"U": U_all.cpu().numpy()[keep], "u0": u0_all.cpu().numpy()[keep]}
        else:
            outs = {"U": U[:B].cpu().numpy(), "u0": u0[:B].cpu().numpy()}
        if env_step:
            outs["x0"] = x0.cpu().numpy()
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in outs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), np.ascontiguousarray(a, np.float32))

    if rank == 0:
        solves_per_step = max(n_stream, 1)
        units = G * cfg.K * cfg.H * args.steps * solves_per_step
        value = units / elapsed
        ms_step = elapsed / args.steps * 1e3
        avg_roll_s = (us_roll / max(n_roll, 1)) * 1e-6
        # the arithmetic the path actually ran: the analytic cartpole is fp32 whatever --precision says; the split
        # mode names the CA's layer 1 when the engine's probe gave it two products (bf16x3, layer 1 bf16x2: W_hi a_hi
        # + W_lo a_hi, include/mppi.h MPPI_PREC_BF16X3), or the fp16 form ran (mppi_x3_f16): the per-wave kernels'
        # "f16x2w/l1:f16x1" = layer 0, the statistic and the last layer as fp16 W hi + lo against one fp16 operand, layer
        # 1 one fp16 product; "bf16x3/l1:f16x1,l2:f16x2w" with layer 0 and the statistic bf16x3 (MPPI_X3_F16_L0=0)
        dtype = "fp32" if (cfg.precision == 0 or spec["bound"] == "hbm") else ("bf16x3" if cfg.precision == 2 else "bf16")
        if dtype == "bf16x3" and f16_all:
            dtype_label = "f16x2w/l1:f16x1" + (",l2:f16x1" if f16_l2x1 else "")
        elif dtype == "bf16x3" and f16_l1:
            dtype_label = "bf16x3/l1:f16x1,l2:" + ("f16x1" if f16_l2x1 else "f16x2w")
        else:
            dtype_label = dtype + ("/l1:bf16x2" if dtype == "bf16x3" and l1_products == 2 else "")
        # the roofline kernel: the workload's rollout kernel the engine actually ran (kernel trace: the longest of its
        # aliases, e.g. fc_pipe_kernel for whole rounds of tiles)
        kname = workload_kernel(args.workload)
        if ktr:
            cands = [(ms, k) for k, ms in ktr.items() if any(al in k for al in KERNEL_ALIASES.get(kname, (kname,)))]
            if cands:
                kname = max(cands)[1].split("<")[0].split(" ")[0]
        if spec["bound"] == "mfma":
            flop = B * cfg.K * cfg.H * spec["flop"]
            # the split mode's algorithmic FLOP (the net's own, fp32-accurate) is priced against the dense bf16 MFMA
            # peak, the matrix hardware it runs on; its products are two or three bf16 MFMAs each, so its ceiling is
            # peak / m, m = the kernel's MFMAs per bf16-equivalent product, reported beside it (frac_of_split_ceiling)
            peak = PEAK_BF16 if dtype in ("bf16", "bf16x3") else PEAK_FP32
            roof = dict(bound="mfma", achieved=flop / avg_roll_s / 1e12, peak=peak / 1e12, unit="TFLOP/s",
                        frac=(flop / avg_roll_s) / peak, traffic=None,
                        kernel=kname, avg_launch_us=avg_roll_s * 1e6,
                        launches=n_roll, per_launch=f"{B}x{cfg.K}x{cfg.H} sample-steps x {spec['flop']} FLOP")
            if dtype == "bf16x3":
                # the CA's layer 1 takes two products when the engine's probe of the loaded weights allows it
                # (mppi_x3_layer1): the per-wave kernels then issue 242 MFMAs per wave-step for the 102 of the bf16
                # form, the M-split kernel 136 for 56; three products everywhere else (longer horizons, the MLP); the
                # fp16 form (mppi_x3_f16) fewer, below (fp16 MFMAs: the same dense peak as bf16)
                two = l1_products == 2
                per_wave = routed.startswith(("fc_wave32_x3p_kernel", "fc_wave32_x3_kernel"))
                # fp16 form, per-wave kernels: statistic 12, layer 0 32 (fc_wave32_x3p_kernel 28: the qvel rows' first
                # k-step as one product), layer 1 64, the last layer 32 (one product: 16) per wave-step for 102;
                # fc_rollout_kernel_x3d / _x3h: layer 0 16, layer 1 16, the last layer 8 (4) for 28
                l2 = (16 if per_wave else 4) if f16_l2x1 else (32 if per_wave else 8)
                l0 = 28 if routed.startswith("fc_wave32_x3p_kernel") else 32
                if f16_all and per_wave:
                    m = (12 + l0 + 64 + l2) / 102
                elif f16_all:
                    m = (16 + 16 + l2) / 28
                elif f16_l1 and per_wave:
                    m = (18 + 48 + 64 + l2) / 102
                elif f16_l1:
                    m = (24 + 16 + l2) / 28
                elif two and per_wave:
                    m = 242 / 102
                elif two:
                    m = 136 / 56
                else:
                    m = 3.0
                roof["split_mfma_per_product"] = round(m, 4)
                roof["frac_of_split_ceiling"] = (flop / avg_roll_s) / (PEAK_BF16 / m)
                roof["peak_note"] = ("peak = dense bf16 (= fp16) MFMA peak; each fp32-accurate product is one to three "
                                     "bf16 / fp16 MFMAs (hi/lo splits), so frac_of_split_ceiling prices the same rate "
                                     "against peak / split_mfma_per_product")
        else:
            nbytes = 2 * B * cfg.K * cfg.H * cfg.nu * 4 + 2 * B * cfg.K * 4 + 2 * B * cfg.H * cfg.nu * 4
            roof = dict(bound="hbm", achieved=nbytes / avg_roll_s / 1e9, peak=PEAK_HBM / 1e9, unit="GB/s",
                        frac=(nbytes / avg_roll_s) / PEAK_HBM, traffic=None, kernel=kname,
                        avg_launch_us=avg_roll_s * 1e6, launches=n_roll, per_launch=f"{nbytes} algorithmic bytes")
        roof["timing"] = ("device wall clock (s_memrealtime, mppi_kernel_clock): first block start to last block end "
                          f"of each of the {n_roll} rollout launches inside the timed region, averaged")
        if kname == "fal_gemm_kernel":
            roof["timing"] += ("; the layer-by-layer FA rollout is a chain of 1 + 5 x layers launches per horizon step "
                               "plus a finish launch, stamped as one: its first kernel's first block start to the "
                               "finish kernel's last block end")
        if tr is not None:
            roof["traffic"] = tr["bytes"]
            roof["traffic_note"] = (f"rocprofv3 PMC per launch of {tr['kernel']}: FETCH_SIZE {tr['fetch_kb']:.0f} KB "
                                    f"(x{tr['factor']:g}, see bench.py FETCH_FACTOR), "
                                    f"WRITE_SIZE {tr['write_kb']:.0f} KB")
        cpu = None
        if not args.no_cpu_baseline and world == 1:
            cpu = cpu_baseline(args.workload, spec, threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)))
        line = {
            "metric": METRIC, "value": value, "unit": "trajectory-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_step, "higher_is_better": True,
            "scaling": "strong" if spec.get("global_solves") else "weak",
            "vs_baseline": None, "dtype": dtype_label,
            "data": "synthetic: device Philox noise; x0 from logged states; trained or seeded weights",
            "config": {"workload": args.workload, "desc": spec["desc"], "K": cfg.K, "H": cfg.H,
                       "solves_per_gpu": B * solves_per_step, "global_solves": G * solves_per_step,
                       "ms_per_solve": ms_step / solves_per_step,  # B solves run concurrently
                       "parallelism": (f"dp{world} (independent solves, RCCL all-gather of every step's U*, u0, "
                                       f"{args.gather_every} steps per collective, overlapped with the next solves)"
                                       if gather is not None else
                                       "dp1 (independent solves; the RCCL all-gather of U*, u0 runs at N > 1)"),
                       "launch": launch, "rollout_kernel": routed,
                       **({"x3_layer1_products": l1_products, "x3_layer1_probe_rel_err": l1_probe,
                           "x3_f16_form": f16_ran, "x3_f16_probe_rel_err": f16_probe}
                          if dtype == "bf16x3" and args.workload.startswith("humanoid_ca") else {})},
            "kernel_ms": ktr,
            "kernel_timing": ("kernel_ms: average duration per launch of each kernel of the timed region's path "
                              "(graph replays or chained solves, config.launch) from a rocprofv3 --kernel-trace pass "
                              "of this command without the plain-solve pass, after the same clock ramp, over its "
                              "last 6 steps; "
                              "plain_solve_kernel_ms: HIP events on the engine's stream around 16 plain solves "
                              "(noise_kernel, rollout, block-local reduce) before the timed region"),
            "plain_solve_kernel_ms": None if prof_kt is None else {k: (v[1] / max(v[0], 1)) for k, v in prof_kt.items()},
            "roofline": roof,
            "gpu_ramp": f"{n_ramp} untimed steps ({args.ramp_ms:g} ms) before the {args.warmup} warmup steps",
            **({"gather": "RCCL all-gather forced at world 1 (MPPI_FORCE_GATHER)"} if force_gather and world == 1
               else {}),
            "cpu_baseline": cpu,
        }
        print(json.dumps(line))
    if world > 1 or force_gather:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
