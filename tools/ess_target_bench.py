"""Cost of ESS targeting (mppi_set_ess_target) on one GPU, as JSON lines.

    python tools/ess_target_bench.py [--repeats 5] [--steps 40]

Per shape -- BASELINE config #4 (64 humanoid CrossAttention solves), its 8-solve shard, and config #2 (the analytic
cartpole; bench.py's workloads) -- arms alternated on one handle, device events around a run of chained steps
(MPPI_FLAG_CHAIN), medians of the repeats:

  chained          targeting off: the yardstick (the cartpole in its fused one-launch form)
  chained_ess      targeting on (ess_frac 0.1, bounds 1e-3 .. 1e3): the yardstick's launches plus lambda_search_kernel
                   with 15 candidates per pass; the cartpole then runs rollout + search + reduce_kernel (3 launches)
  chained_bisect   the same with MPPI_LAMBDA_SEARCH=bisect (one candidate per pass)
  chained_pinned   targeting on with lambda_min = lambda_max = the configured lambda: the search's two end evaluations
                   only -- for the cartpole, the price of leaving the fused epilogue without a search to speak of

and, from a profiled run of the chained_ess / chained_bisect arms, mppi_kernel_time("lambda") per launch (hipEvents
around the launch: an upper bound that includes the events' own gaps).

A library without mppi_set_ess_target (an older build of this project, selected with MPPI_HIP_LIB) runs the yardstick
alone: the same-box figure of the parent commit.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "humanoid_mppi-rl_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    import torch
    import bench
    import mppi_hip
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a stream of its own: the engine's launches and the events share it
    n, frac, limits = args.steps, 0.1, (1e-3, 1e3)

    for name, workload, solves in (("config4", "humanoid_ca", 64), ("config4, 8-solve shard", "humanoid_ca", 8),
                                   ("config2", "cartpole", 0)):
        spec = bench.workload_spec(workload, bench.DEFAULT_PRECISION.get(workload, "bf16"), solves)
        cfg, B = spec["cfg"], spec["B"]
        eng = mppi_hip.Engine(cfg, device=0)
        eng.load_dynamics(*spec["dyn"]).set_cost(spec["cost"])
        eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        x0 = torch.from_numpy(np.ascontiguousarray(spec["x0_all"][:B], np.float32)).to(dev)
        U = torch.zeros(B, cfg.nu, cfg.H, device=dev)
        u0 = torch.zeros(B, cfg.nu, device=dev)
        has_ess = hasattr(eng.lib, "mppi_set_ess_target")

        def step():
            eng.solve_device(B, x0.data_ptr(), U.data_ptr(), None, seed=7, u0_ptr=u0.data_ptr(), shift=True, chain=True)

        def timed_events(warm=6):
            for i in range(warm + n):
                if i == warm:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                step()
            e1.record()
            torch.cuda.synchronize(dev)
            return 1e3 * e0.elapsed_time(e1) / n

        def arm(target, bisect=False):
            def run():
                if has_ess:
                    eng.set_ess_target(*target)
                if bisect:
                    os.environ["MPPI_LAMBDA_SEARCH"] = "bisect"
                try:
                    return timed_events()
                finally:
                    os.environ.pop("MPPI_LAMBDA_SEARCH", None)
            return run

        arms = {"chained": arm((0.0, *limits))}
        if has_ess:
            arms.update(chained_ess=arm((frac, *limits)), chained_bisect=arm((frac, *limits), bisect=True),
                        chained_pinned=arm((frac, cfg.lambda_, cfg.lambda_)))
        res = {k: [] for k in arms}
        for _ in range(args.repeats):  # alternated: every repeat visits every arm
            for k, f in arms.items():
                res[k].append(f())
        med = {k: statistics.median(v) for k, v in res.items()}
        out = {"what": "us_per_step", "config": name, "B": B, "K": cfg.K, "H": cfg.H, "steps": n, "runs": res,
               "median": med}
        if has_ess:
            out["ess_minus_off_us"] = med["chained_ess"] - med["chained"]
            out["bisect_minus_off_us"] = med["chained_bisect"] - med["chained"]
            out["pinned_minus_off_us"] = med["chained_pinned"] - med["chained"]
            for key, bisect in (("lambda_kernel_us", False), ("lambda_kernel_bisect_us", True)):
                eng.set_ess_target(frac, *limits)
                if bisect:
                    os.environ["MPPI_LAMBDA_SEARCH"] = "bisect"
                try:
                    for _ in range(6):
                        step()
                    eng.profile(True)
                    for _ in range(n):
                        step()
                    eng.sync()
                    cnt, ms = eng.kernel_time("lambda")
                    eng.profile(False)
                finally:
                    os.environ.pop("MPPI_LAMBDA_SEARCH", None)
                out[key] = 1e3 * ms / max(cnt, 1)
            out["lambda"] = [float(v) for v in eng.lambdas(min(B, 4))]
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
