"""Cost of adapting the sampling law on the device (mppi_set_noise_adapt) on one GPU, as JSON lines.

    python tools/noise_adapt_bench.py [--repeats 5] [--steps 40]

Per shape -- BASELINE config #4 (64 humanoid CrossAttention solves, K = 1024, H = 64), its 8-solve shard, and config
#2 (analytic cartpole, K = 4096, H = 50; bench.py's workloads), each with an active model (rho = 0.5, sigma_u = the
preset's sigma) -- arms alternated on one handle, device events (or, for the host loop, the wall clock) around a run
of steps, medians of the repeats:

  chained_stats   chained steps (MPPI_FLAG_CHAIN) with MPPI_FLAG_STATS, adaptation off: the yardstick
  chained_adapt   the same with adaptation on: the yardstick's launches plus the one-wave noise_adapt_kernel
  graph_adapt     one captured graph of `steps` adapting solves
  host_loop       the host-adapting loop: plain counter solve with the flag, Engine.stats (waits for the stream),
                  stats.adapt_noise_model, Engine.set_noise_model

A library without mppi_set_noise_adapt (an older build of this project) runs the arms it has: chained_stats and
host_loop.
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    from mppi_hip.stats import adapt_noise_model
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a stream of its own: the engine's launches and the events share it
    n, rate, limits = args.steps, 0.1, (1e-3, 10.0, 0.95)

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
        has_adapt = hasattr(eng, "set_noise_adapt")
        law0 = (np.full(cfg.nu, cfg.sigma, np.float32), 0.5)

        def reset(adapt):
            eng.set_noise_model(*law0)
            if has_adapt:
                eng.set_noise_adapt(rate if adapt else 0.0, *limits)

        def timed_events(step, warm=6):
            for i in range(warm + n):
                if i == warm:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                step()
            e1.record()
            torch.cuda.synchronize(dev)
            return 1e3 * e0.elapsed_time(e1) / n

        def chained(flag):
            return lambda: eng.solve_device(B, x0.data_ptr(), U.data_ptr(), None, seed=7, u0_ptr=u0.data_ptr(),
                                            shift=True, chain=True, stats=flag)

        def arm_chained_stats():
            reset(False)
            return timed_events(chained(True))

        def arm_chained_adapt():
            reset(True)
            return timed_events(chained(False))

        def arm_graph_adapt():
            reset(True)
            eng.graph_capture(B, n, x0.data_ptr(), U.data_ptr(), u0.data_ptr(), seed=7, shift=True, env_step=False)
            eng.graph_launch(sync=True)  # warm
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.graph_launch(sync=False)
            e1.record()
            torch.cuda.synchronize(dev)
            return 1e3 * e0.elapsed_time(e1) / n

        def arm_host_loop():
            reset(False)
            law = [law0[0].astype(np.float64), law0[1]]

            def step():
                eng.solve_device(B, x0.data_ptr(), U.data_ptr(), None, seed=7, u0_ptr=u0.data_ptr(), shift=True,
                                 seed_counter=True, stats=True)
                st = eng.stats(B)
                if np.all(st["n_finite"] > 0):
                    law[0], law[1] = adapt_noise_model(law[0], law[1], st["eps_m2"], st["eps_m11"], rate, *limits)
                    eng.set_noise_model(law[0], law[1])

            for _ in range(6):
                step()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                step()
            torch.cuda.synchronize(dev)
            return 1e6 * (time.perf_counter() - t0) / n

        arms = {"chained_stats": arm_chained_stats, "host_loop": arm_host_loop}
        if has_adapt:
            arms.update(chained_adapt=arm_chained_adapt, graph_adapt=arm_graph_adapt)
        res = {k: [] for k in arms}
        for _ in range(args.repeats):  # alternated: every repeat visits every arm
            for k, f in arms.items():
                res[k].append(f())
        med = {k: statistics.median(v) for k, v in res.items()}
        out = {"what": "us_per_step", "config": name, "B": B, "nu": cfg.nu, "steps": n, "runs": res, "median": med}
        if has_adapt:
            out["adapt_minus_stats_us"] = med["chained_adapt"] - med["chained_stats"]
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
