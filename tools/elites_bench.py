"""Cost of elite truncation (mppi_set_elites) on one GPU beside the lambda search, as JSON lines.

    python tools/elites_bench.py [--repeats 5] [--calls 30] [--steps 20] [--no-step]

  kernels   per shape -- BASELINE config #4's costs (B = 64, K = 1024), its 8-solve shard (B = 8), config #5's K = 8192
            (B = 1) and B = 1 at K = 32768 -- mppi_profile events around the launches of mppi_elites_eval ("elites") and
            of mppi_lambda_eval ("lambda", ess_frac 0.1, bounds 1e-3 .. 1e3: the yardstick, one block per solve with
            the costs in registers, like the selection) in one process on the same staging cost buffer: Gaussian costs
            50 +- 10, and the same rounded to quarters (many duplicates).  n_elite = K / 10 and K / 2.  The arms are
            alternated --repeats times, --calls launches each after a ramp; medians, microseconds per launch.  Events
            bracket one launch each, so a figure includes the events' own gaps: an upper bound, alike for every arm.
  step      config #4 as one captured graph of --steps chained solves (shift), replayed; device events around the
            replay, microseconds per solve; elites off and on (K / 10), alternated, medians.

--trace runs only the evaluations (no events, nothing printed but the shape): 30 launches each of the lambda search
and the selection on the Gaussian costs, at n_elite = K / 10 and at K / 2 -- the run to put under
`rocprofv3 --kernel-trace --stats`, one shape per run (--only), for the kernels' own durations
(scripts/elites_trace.sh).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "humanoid_mppi-rl_amd")]

SHAPES = (("config4", 64, 1024), ("config4, 8-solve shard", 8, 1024), ("config5", 1, 8192), ("kMaxK", 1, 32768))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    ap.add_argument("--only", default=None, help="one shape by name: config4, config4-shard, config5, kMaxK")
    ap.add_argument("--trace", action="store_true", help="only the evaluations, for a kernel trace")
    args = ap.parse_args()
    import torch
    import bench
    import mppi_hip
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a stream of its own: the step arm's launches and events share it

    for name, B, K in SHAPES:
        if args.only and args.only != name.replace(", 8-solve ", "-"):
            continue
        if args.trace:
            eng = mppi_hip.Engine(mppi_hip.Config(nx=4, nu=1, H=2, K=K, max_batch=B, lambda_=1.0), device=0)
            eng.set_ess_target(0.1, 1e-3, 1e3)
            costs = (50.0 + 10.0 * np.random.RandomState(K + B).randn(B, K)).astype(np.float32)
            for n_elite in (max(1, K // 10), K // 2):
                eng.set_elites(n_elite)
                for _ in range(30):
                    eng.lambda_eval(costs)
                    eng.elites_eval(costs)
            print(json.dumps({"config": name, "B": B, "K": K}), flush=True)
            eng.close()
            continue
        eng = mppi_hip.Engine(mppi_hip.Config(nx=4, nu=1, H=2, K=K, max_batch=B, lambda_=1.0), device=0)
        eng.set_ess_target(0.1, 1e-3, 1e3)
        gauss = (50.0 + 10.0 * np.random.RandomState(K + B).randn(B, K)).astype(np.float32)
        for data, costs in (("gauss", gauss), ("quantised", (np.round(gauss * 4.0) / 4.0).astype(np.float32))):
            def timed(key, call):
                for _ in range(10):  # clock ramp
                    call()
                eng.profile(True)
                for _ in range(args.calls):
                    call()
                cnt, ms = eng.kernel_time(key)
                eng.profile(False)
                return 1e3 * ms / max(cnt, 1)

            for n_elite in (max(1, K // 10), K // 2):
                eng.set_elites(n_elite)
                arms = {"lambda": lambda: timed("lambda", lambda: eng.lambda_eval(costs)),
                        "elites": lambda: timed("elites", lambda: eng.elites_eval(costs))}
                runs = {k: [] for k in arms}
                for _ in range(args.repeats):  # alternated: every repeat visits every arm
                    for k, f in arms.items():
                        runs[k].append(f())
                med = {k: statistics.median(v) for k, v in runs.items()}
                out = {"what": "kernel_us", "config": name, "B": B, "K": K, "data": data, "n_elite": n_elite,
                       "calls": args.calls, "median": med, "runs": runs,
                       "elites_over_lambda": med["elites"] / med["lambda"]}
                print(json.dumps(out), flush=True)
        eng.close()

    if args.no_step or args.trace or (args.only and args.only != "config4"):
        return
    n = args.steps
    spec = bench.workload_spec("humanoid_ca", bench.DEFAULT_PRECISION.get("humanoid_ca", "bf16"), 64)
    cfg, B = spec["cfg"], spec["B"]
    eng = mppi_hip.Engine(cfg, device=0)
    eng.load_dynamics(*spec["dyn"]).set_cost(spec["cost"])
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    x0 = torch.from_numpy(np.ascontiguousarray(spec["x0_all"][:B], np.float32)).to(dev)
    U = torch.from_numpy((0.1 * np.random.RandomState(0).randn(B, cfg.nu, cfg.H)).astype(np.float32)).to(dev)
    u0 = torch.zeros(B, cfg.nu, device=dev)

    def replay(n_elite):
        eng.set_elites(n_elite)
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

    arms = {"off": 0, "elites": cfg.K // 10}
    res = {k: [] for k in arms}
    for _ in range(args.repeats):  # alternated: every repeat visits every arm
        for k, v in arms.items():
            res[k].append(replay(v))
    out = {"what": "step_us", "config": "config4", "B": B, "K": cfg.K, "H": cfg.H, "steps": n,
           "median": {k: statistics.median(v) for k, v in res.items()}, "runs": res}
    out["elites_minus_off_us"] = out["median"]["elites"] - out["median"]["off"]
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
