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

  population  (--population; mppi_set_population) config #4 at n_iter = 3 as the same captured graph under the tables
            (1024, 1024, 1024) -- the feature off --, (1024, 768, 576) and (1024, 512, 256), each with the next noise at
            another pitch drawn by the two-pitch reduce (the default) and by a launch of its own behind the reduce
            (MPPI_GEN_TWO_PITCH=0), alternated in one process, medians.  The yardstick of a table, measured in the same
            run, is the sum of the n_iter = 1 graph steps of three handles at its sample counts: what the defining loop
            would cost without host round trips (with three shifts and env steps, not one: it is not the code under
            test).  Then, kernel for kernel with mppi_profile events on chained steps at n_iter = 2 (MPPI_GEN_OVERLAP=0):
            the "reduce" and "noise" time per control step of (1024, 1024) -- reduce_kernel<GEN> at one pitch --,
            (1024, 512) and (1024, 256) with the two-pitch form at both boundaries, at the shrink alone, at the growth
            alone (MPPI_GEN_TWO_PITCH=shrink|grow) and at neither.

--trace runs only the evaluations (no events, nothing printed but the shape): 20 launches each of the selection and
the tracking kernel on the same inputs -- the run to put under `rocprofv3 --kernel-trace --stats`, or under one
`rocprofv3 --pmc` pass, one shape per run (--only), for the kernels' own durations and counters
(scripts/iterations_trace.sh).
"""
import argparse
import dataclasses
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
    ap.add_argument("--population", action="store_true", help="only the population-size decay arms")
    args = ap.parse_args()
    import torch
    import bench
    import mppi_hip
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a stream of its own: the step arm's launches and events share it

    if args.population:
        return population(args, torch, bench, mppi_hip, dev)
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


POP_TABLES = ((1024, 1024, 1024), (1024, 768, 576), (1024, 512, 256))


def _pop_engine(torch, bench, mppi_hip, dev, K=None):
    spec = bench.workload_spec("humanoid_ca", bench.DEFAULT_PRECISION.get("humanoid_ca", "bf16"), 64)
    cfg, B = spec["cfg"], spec["B"]
    if K is not None and K != cfg.K:
        cfg = dataclasses.replace(cfg, K=K)
    eng = mppi_hip.Engine(cfg, device=0)
    eng.load_dynamics(*spec["dyn"]).set_cost(spec["cost"])
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    x_start = np.ascontiguousarray(spec["x0_all"][:B], np.float32)
    U_start = (0.1 * np.random.RandomState(0).randn(B, cfg.nu, cfg.H)).astype(np.float32)
    t = dict(x_start=x_start, U_start=U_start, x0=torch.from_numpy(x_start.copy()).to(dev),
             U=torch.from_numpy(U_start.copy()).to(dev), u0=torch.zeros(B, cfg.nu, device=dev))
    return eng, cfg, B, t


def population(args, torch, bench, mppi_hip, dev):
    n = args.steps
    knob = "MPPI_GEN_TWO_PITCH"

    def reset(t):
        t["x0"].copy_(torch.from_numpy(t["x_start"]))  # every arm from the same state and nominal
        t["U"].copy_(torch.from_numpy(t["U_start"]))

    def replay(eng, B, t):
        eng.graph_launch(sync=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            eng.graph_launch(sync=False)
        e1.record()
        torch.cuda.synchronize(dev)
        return 1e3 * e0.elapsed_time(e1) / (3 * n)

    def set_knob(v):
        os.environ.pop(knob, None)
        if v is not None:
            os.environ[knob] = v

    eng, cfg, B, t = _pop_engine(torch, bench, mppi_hip, dev)
    ks = sorted({k for tab in POP_TABLES for k in tab})
    singles = {k: _pop_engine(torch, bench, mppi_hip, dev, K=k) for k in ks}

    def table_arm(tab, sep):
        reset(t)
        set_knob("0" if sep else None)
        eng.set_iterations(len(tab))
        eng.set_population(tab)
        eng.graph_capture(B, n, t["x0"].data_ptr(), t["U"].data_ptr(), t["u0"].data_ptr(), seed=7, shift=True,
                          env_step=True)
        set_knob(None)
        return replay(eng, B, t)

    def single_arm(k):
        e, _, b, tt = singles[k]
        reset(tt)
        e.graph_capture(b, n, tt["x0"].data_ptr(), tt["U"].data_ptr(), tt["u0"].data_ptr(), seed=7, shift=True,
                        env_step=True)
        return replay(e, b, tt)

    arms = {}
    for tab in POP_TABLES:
        arms["x".join(map(str, tab))] = lambda tab=tab: table_arm(tab, False)
        if len(set(tab)) > 1:
            arms["x".join(map(str, tab)) + "_separate"] = lambda tab=tab: table_arm(tab, True)
    for k in ks:
        arms[f"single_{k}"] = lambda k=k: single_arm(k)
    res = {k: [] for k in arms}
    for _ in range(args.repeats):  # alternated: every repeat visits every arm
        for k, f in arms.items():
            res[k].append(f())
    med = {k: statistics.median(v) for k, v in res.items()}
    yard = {"x".join(map(str, tab)): sum(med[f"single_{k}"] for k in tab) for tab in POP_TABLES}
    kernels = [eng.iter_rollout_kernel(i) for i in range(3)]
    print(json.dumps({"what": "population_step_us", "config": "config4", "B": B, "K": cfg.K, "H": cfg.H, "steps": n,
                      "median": med, "runs": res, "yardstick_sum_of_single_steps_us": yard,
                      "minus_yardstick_us": {k: med[k] - yard[k] for k in yard},
                      "last_table_kernels": kernels}), flush=True)
    for e, _, _, _ in singles.values():
        e.close()

    # kernel for kernel: chained steps at n_iter = 2, every next noise inside or behind the reduce
    os.environ["MPPI_GEN_OVERLAP"] = "0"
    eng.set_population(None)
    eng.set_iterations(2)

    def chain_arm(tab, v):
        reset(t)
        set_knob(v)
        eng.set_population(tab)
        call = lambda: eng.solve_device(B, t["x0"].data_ptr(), t["U"].data_ptr(), None, seed=7,
                                        u0_ptr=t["u0"].data_ptr(), shift=True, env_step=True, chain=True)
        for _ in range(3):  # clock ramp (and the prime)
            call()
        eng.profile(True)
        for _ in range(args.calls):
            call()
        torch.cuda.synchronize(dev)
        out = {k: 1e3 * eng.kernel_time(k)[1] / args.calls for k in ("reduce", "noise")}
        eng.profile(False)
        set_knob(None)
        return out

    karms = {"1024x1024": ((1024, 1024), None)}
    for k2 in (512, 256):
        for name, v in (("both", None), ("shrink_only", "shrink"), ("grow_only", "grow"), ("separate", "0")):
            karms[f"1024x{k2}_{name}"] = ((1024, k2), v)
    kres = {k: {"reduce": [], "noise": []} for k in karms}
    for _ in range(args.repeats):
        for k, (tab, v) in karms.items():
            o = chain_arm(tab, v)
            for kk in o:
                kres[k][kk].append(o[kk])
    kmed = {k: {kk: statistics.median(v) for kk, v in d.items()} for k, d in kres.items()}
    for k in kmed:
        kmed[k]["reduce_plus_noise"] = kmed[k]["reduce"] + kmed[k]["noise"]
    print(json.dumps({"what": "population_reduce_us_per_step", "config": "config4", "B": B, "n_iter": 2,
                      "calls": args.calls, "median": kmed, "runs": kres}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
