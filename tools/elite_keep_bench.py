"""Cost of keep / shift elites (mppi_set_elite_keep) on one GPU beside the control-cost term kernel, as JSON lines.

    python tools/elite_keep_bench.py [--repeats 3] [--calls 10] [--steps 20] [--no-step] [--only SHAPE]

  kernels   per shape -- BASELINE config #4 (B = 64, nu = 21, H = 64, K = 1024), its 8-solve shard (B = 8), config #5
            (B = 1, H = 128, K = 8192) and config #2 (B = 1, nu = 1, H = 50, K = 4096) -- mppi_profile events around the
            launches of mppi_keep_store_eval ("keep": the selection + the gather), mppi_elites_eval at the same n
            ("elites": the selection alone, so keep - elites is the gather with one event gap less),
            mppi_keep_inject_eval ("keep": the inject kernel on a full set) and mppi_control_term_eval ("ctrl_cost": the
            yardstick, one streaming pass over the same staging noise buffer) in one process.  n_keep = K / 32 and
            K / 8.  The arms are alternated --repeats times, --calls launches each after a ramp; medians, microseconds
            per launch.  Events bracket one launch group each, so a figure includes the events' own gaps: an upper
            bound, alike for every arm.
  step      the shape's workload as one captured graph of --steps chained solves (shift), replayed; device events around
            the replay, microseconds per solve; the feature off and on (K / 32, K / 8), alternated, medians.  (The
            analytic cartpole of config #2 leaves its fused one-launch form while the feature is on.)

--trace runs only the evaluations (no events, nothing printed but the shape): 20 launches each of the control-cost
term, the store and the injection at n_keep = K / 32 and K / 8 -- the run to put under `rocprofv3 --kernel-trace
--stats`, one shape per run (--only), for the kernels' own durations (scripts/elite_keep_trace.sh).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "humanoid_mppi-rl_amd")]

# name, B, nu, H, K, (bench.py workload, per-rank solves) of the step arm
SHAPES = (("config4", 64, 21, 64, 1024, ("humanoid_ca", 64)), ("config4-shard", 8, 21, 64, 1024, ("humanoid_ca", 8)),
          ("config5", 1, 21, 128, 8192, ("humanoid_ca_stream", 0)), ("config2", 1, 1, 50, 4096, ("cartpole", 0)))


def kernels(args, mppi_hip, name, B, nu, H, K):
    eng = mppi_hip.Engine(mppi_hip.Config(nx=4, nu=nu, H=H, K=K, max_batch=B, lambda_=1.0, sigma=0.5), device=0)
    eng.set_control_cost(0.05)
    rs = np.random.RandomState(K + B)
    U = (0.1 * rs.randn(B, nu, H)).astype(np.float32)
    noise = np.float32(0.5) * np.random.default_rng(K + B).standard_normal((B, nu, H, K), dtype=np.float32)
    costs = (50.0 + 10.0 * rs.randn(B, K)).astype(np.float32)
    for n_keep in (K // 32, K // 8):
        eng.set_elite_keep(n_keep)
        eng.set_elites(n_keep)
        v, _, _, count, steps = eng.keep_store_eval(U, noise, costs, shift=True)

        calls = {"ctrl_cost": ("ctrl_cost", lambda: eng.control_term_eval(U, noise)),
                 "store": ("keep", lambda: eng.keep_store_eval(U, noise, costs, shift=True)),
                 "select": ("elites", lambda: eng.elites_eval(costs)),
                 "inject": ("keep", lambda: eng.keep_inject_eval(U, noise, v, count, steps))}
        if args.trace:
            for _ in range(20):
                for _, call in calls.values():
                    call()
            continue

        def timed(key, call):
            for _ in range(3):  # clock ramp
                call()
            eng.profile(True)
            for _ in range(args.calls):
                call()
            cnt, ms = eng.kernel_time(key)
            eng.profile(False)
            return 1e3 * ms / max(cnt, 1)

        runs = {k: [] for k in calls}
        for _ in range(args.repeats):  # alternated: every repeat visits every arm
            for k, (key, call) in calls.items():
                runs[k].append(timed(key, call))
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({"what": "kernel_us", "config": name, "B": B, "nu": nu, "H": H, "K": K, "n_keep": n_keep,
                          "calls": args.calls, "median": med, "runs": runs,
                          "gather_us": med["store"] - med["select"],
                          "gather_over_ctrl_cost": (med["store"] - med["select"]) / med["ctrl_cost"]}), flush=True)
    if args.trace:
        print(json.dumps({"config": name, "B": B, "K": K}), flush=True)
    eng.close()


def step(args, torch, bench, mppi_hip, name, workload, solves):
    dev = torch.device("cuda", 0)
    n = args.steps
    spec = bench.workload_spec(workload, bench.DEFAULT_PRECISION.get(workload, "bf16"), solves)
    cfg, B = spec["cfg"], spec["B"]
    eng = mppi_hip.Engine(cfg, device=0)
    eng.load_dynamics(*spec["dyn"]).set_cost(spec["cost"])
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    x0 = torch.from_numpy(np.ascontiguousarray(spec["x0_all"][:B], np.float32).reshape(B, cfg.nx)).to(dev)
    U = torch.from_numpy((0.1 * np.random.RandomState(0).randn(B, cfg.nu, cfg.H)).astype(np.float32)).to(dev)
    u0 = torch.zeros(B, cfg.nu, device=dev)

    def replay(n_keep):
        eng.set_elite_keep(n_keep)
        eng.graph_capture(B, n, x0.data_ptr(), U.data_ptr(), u0.data_ptr(), seed=7, shift=True, env_step=False)
        for _ in range(3):
            eng.graph_launch(sync=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            eng.graph_launch(sync=False)
        e1.record()
        torch.cuda.synchronize(dev)
        return 1e3 * e0.elapsed_time(e1) / (3 * n)

    arms = {"off": 0, "K/32": cfg.K // 32, "K/8": cfg.K // 8}
    res = {k: [] for k in arms}
    for _ in range(args.repeats):  # alternated: every repeat visits every arm
        for k, v in arms.items():
            res[k].append(replay(v))
    out = {"what": "step_us", "config": name, "B": B, "K": cfg.K, "H": cfg.H, "steps": n,
           "median": {k: statistics.median(v) for k, v in res.items()}, "runs": res}
    out["on_minus_off_us"] = {k: out["median"][k] - out["median"]["off"] for k in ("K/32", "K/8")}
    print(json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    ap.add_argument("--no-kernels", action="store_true", help="the graph step alone")
    ap.add_argument("--only", default=None, help="one shape by name: config4, config4-shard, config5, config2")
    ap.add_argument("--trace", action="store_true", help="only the evaluations, for a kernel trace")
    args = ap.parse_args()
    import torch
    import bench
    import mppi_hip
    torch.cuda.set_stream(torch.cuda.Stream(torch.device("cuda", 0)))  # the step arm's launches and events share it
    for name, B, nu, H, K, (workload, solves) in SHAPES:
        if args.only and args.only != name:
            continue
        if not args.no_kernels:
            kernels(args, mppi_hip, name, B, nu, H, K)
        if not (args.no_step or args.trace):
            step(args, torch, bench, mppi_hip, name, workload, solves)


if __name__ == "__main__":
    main()
