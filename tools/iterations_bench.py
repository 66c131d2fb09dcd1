"""Cost of inner iterations per control step (mppi_set_iterations) on one GPU, as JSON lines.

    python tools/iterations_bench.py [--repeats 5] [--calls 10] [--steps 20] [--no-step] [--only config4|kMaxK]

  kernels   per shape -- BASELINE config #4 (B = 64, K = 1024, H = 64, nu = 21) and B = 1 at K = 32768 (same H, nu) --
            mppi_profile events around the launches of mppi_iter_best_eval ("iter": one packed minimum over the costs
            and a gather of nu H = 1344 controls) and of mppi_elites_eval ("elites", n_elite = K / 10: the yardstick, a
            radix selection over the same costs in the same registers) in one process on the same staging buffers:
            Gaussian costs 50 +- 10, unit noise.  The arms are alternated --repeats times, --calls launches each after
            a ramp; medians, microseconds per launch.  Events bracket one launch each, so a figure includes the events'
            own gaps: an upper bound, alike for both arms.
  step      config #4 as one captured graph of --steps control steps (shift + env step), replayed; device events
            around the replay, microseconds per control step; n_iter = 1, n_iter = 1 without the env step, and
            n_iter = 3, alternated in one process, medians.  The yardstick of n_iter = 3 is three n_iter = 1 steps (a
            host loop's cost without its round trips); the line also gives what the two env steps an iterated step does
            not take and the three tracking launches it adds make of the difference.

--trace runs only the evaluations (no events, nothing printed but the shape): 20 launches each of the selection and
the tracking kernel on the same inputs -- the run to put under `rocprofv3 --kernel-trace --stats`, or under one
`rocprofv3 --pmc` pass, one shape per run (--only), for the kernels' own durations and counters
(scripts/iterations_trace.sh).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "humanoid_mppi-rl_amd")]

SHAPES = (("config4", 64, 1024), ("kMaxK", 1, 32768))
H, NU = 64, 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    ap.add_argument("--no-kernels", action="store_true", help="the graph step alone")
    ap.add_argument("--only", default=None, help="one shape by name: config4, kMaxK")
    ap.add_argument("--trace", action="store_true", help="only the evaluations, for a kernel trace or a counter pass")
    args = ap.parse_args()
    import torch
    import bench
    import mppi_hip
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a stream of its own: the step arm's launches and events share it

    for name, B, K in SHAPES:
        if args.no_kernels or (args.only and args.only != name):
            continue
        eng = mppi_hip.Engine(mppi_hip.Config(nx=4, nu=NU, H=H, K=K, max_batch=B, lambda_=1.0), device=0)
        eng.set_elites(max(1, K // 10))
        rs = np.random.RandomState(K + B)
        costs = (50.0 + 10.0 * rs.randn(B, K)).astype(np.float32)
        U = (0.1 * rs.randn(B, NU, H)).astype(np.float32)
        noise = np.random.default_rng(K + B).standard_normal((B, NU, H, K), dtype=np.float32)  # (float32 at once)
        if args.trace:
            for _ in range(20):
                eng.elites_eval(costs)
                eng.iter_best_eval(U, noise, costs)
            print(json.dumps({"config": name, "B": B, "K": K}), flush=True)
            eng.close()
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

        arms = {"elites": lambda: timed("elites", lambda: eng.elites_eval(costs)),
                "iter": lambda: timed("iter", lambda: eng.iter_best_eval(U, noise, costs))}
        runs = {k: [] for k in arms}
        for _ in range(args.repeats):  # alternated: every repeat visits every arm
            for k, f in arms.items():
                runs[k].append(f())
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({"what": "kernel_us", "config": name, "B": B, "K": K, "H": H, "nu": NU, "n_elite": K // 10,
                          "calls": args.calls, "median": med, "runs": runs,
                          "iter_over_elites": med["iter"] / med["elites"]}), flush=True)
        eng.close()

    if args.no_step or args.trace or (args.only and args.only != "config4"):
        return
    n = args.steps
    spec = bench.workload_spec("humanoid_ca", bench.DEFAULT_PRECISION.get("humanoid_ca", "bf16"), 64)
    cfg, B = spec["cfg"], spec["B"]
    eng = mppi_hip.Engine(cfg, device=0)
    eng.load_dynamics(*spec["dyn"]).set_cost(spec["cost"])
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    x_start = np.ascontiguousarray(spec["x0_all"][:B], np.float32)
    x0 = torch.from_numpy(x_start.copy()).to(dev)
    U_start = (0.1 * np.random.RandomState(0).randn(B, cfg.nu, cfg.H)).astype(np.float32)
    U = torch.from_numpy(U_start.copy()).to(dev)
    u0 = torch.zeros(B, cfg.nu, device=dev)

    def replay(n_iter, env_step):
        x0.copy_(torch.from_numpy(x_start))  # every arm from the same state and nominal
        U.copy_(torch.from_numpy(U_start))
        eng.set_iterations(n_iter)
        eng.graph_capture(B, n, x0.data_ptr(), U.data_ptr(), u0.data_ptr(), seed=7, shift=True, env_step=env_step)
        eng.graph_launch(sync=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            eng.graph_launch(sync=False)
        e1.record()
        torch.cuda.synchronize(dev)
        return 1e3 * e0.elapsed_time(e1) / (3 * n)

    arms = {"n_iter_1": (1, True), "n_iter_1_no_env": (1, False), "n_iter_3": (3, True)}
    res = {k: [] for k in arms}
    for _ in range(args.repeats):  # alternated: every repeat visits every arm
        for k, v in arms.items():
            res[k].append(replay(*v))
    med = {k: statistics.median(v) for k, v in res.items()}
    env = med["n_iter_1"] - med["n_iter_1_no_env"]
    out = {"what": "step_us", "config": "config4", "B": B, "K": cfg.K, "H": cfg.H, "steps": n, "median": med,
           "runs": res, "three_n_iter_1_steps_us": 3.0 * med["n_iter_1"],
           "n_iter_3_minus_three_steps_us": med["n_iter_3"] - 3.0 * med["n_iter_1"], "env_step_us": env,
           "tracking_us_per_iteration": (med["n_iter_3"] - 3.0 * med["n_iter_1_no_env"] - env) / 3.0}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
