"""One plan of T targets against T single-target plans run back to back.

A decoupled step needs KG of the same candidates under several targets (each output alone, and usually all
outputs).  The cross and covariance stages do not depend on the target, so a plan of T targets
(dkg_plan_init_targets) runs them once per call and the envelope once per (target, candidate); the baseline is
what the acquisition layer did before: T plans on the same state, each running the whole forward.  Cases:

  headline_fwd_B128    headline workload, forward of 128 candidates, T = 3 (both outputs and "all")
  headline_grad_B1     headline, value + gradient of 1 host candidate through forward_grad_host, T = 3
  headline_grad_B10    the same at 10 candidates
  stress_fwd_B256      stress workload, forward of 256 candidates, T = 4

Both legs in one process on the same DeviceGPState, alternated; a sample is `inner` calls between two device
synchronisations (forward_grad_host synchronises itself), wall time; the figure is the median over --reps samples
after --warmup warm-ups, per call (one call = all T targets).  The two legs' results are compared bit for bit
first.  The forward cases also report the per-stage times of both plans (dkg_plan_time_stage).  Every case runs in
a child process of its own under a time limit, and the first one that fails ends the run.

    python tools/bench_targets.py            # -> profiles/targets/bench_targets.json
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]

# name -> (workload, route, B, targets, calls per sample, time limit of the child in seconds)
CASES = {
    "headline_fwd_B128": ("headline", "forward", 128, (None, 0, 1), 200, 240),
    "headline_grad_B1": ("headline", "grad_host", 1, (None, 0, 1), 100, 240),
    "headline_grad_B10": ("headline", "grad_host", 10, (None, 0, 1), 100, 240),
    "stress_fwd_B256": ("stress", "forward", 256, (None, 0, 1, 2), 50, 420),
}


def run_case(name, reps, warmup):
    import torch

    from dkg_amd.gp_state import DeviceGPState
    from dkg_amd.synthetic import WORKLOADS, make_problem

    if not torch.cuda.is_available():
        raise SystemExit("bench_targets.py needs a ROCm device: there is no CPU timing of a GPU path")
    workload, route, B, targets, inner, _ = CASES[name]
    dev = torch.device("cuda", 0)
    model, D, X, W = make_problem(WORKLOADS[workload])
    X = X[:B].contiguous()
    state = DeviceGPState(model, D, device=dev)
    T, d, grad = len(targets), X.shape[1], route == "grad_host"
    singles = [state.plan(W, t, B, grad=grad) for t in targets]
    joint = state.plan(W, None, B, grad=grad, targets=targets)
    Xd = X.to(dev)
    kg_s = torch.empty(T, B, dtype=torch.double, device=dev)
    kg_j = torch.empty(T, B, dtype=torch.double, device=dev)

    if grad:
        def leg_singles():
            return [p.forward_grad_host(X) for p in singles]

        def leg_joint():
            return joint.forward_grad_host(X)

        a, b = leg_singles(), leg_joint()
        same = (torch.equal(torch.stack([r[0] for r in a]), b[0]) and torch.equal(torch.stack([r[1] for r in a]), b[1]))
    else:
        def leg_singles():
            for tau, p in enumerate(singles):
                p.forward_into(Xd, kg_s[tau])

        def leg_joint():
            joint.forward_into(Xd, kg_j)

        leg_singles()
        leg_joint()
        torch.cuda.synchronize()
        same = torch.equal(kg_s, kg_j)
    if not same:
        raise SystemExit(f"{name}: the T-target plan and the single-target plans differ")

    legs = {"single_target_plans": leg_singles, "one_plan_of_T_targets": leg_joint}
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e6 / inner)
    res = {"workload": workload, "route": route, "B": B, "targets": ["all" if t is None else t for t in targets],
           "T": T, "m": state.m, "N": state.N, "S": W.shape[0], "calls_per_sample": inner, "bit_equal": True}
    for k, v in times.items():
        res[k] = {"median_us_per_call": statistics.median(v), "min_us_per_call": min(v), "samples": len(v)}
    res["ratio_singles_over_one_plan"] = (res["single_target_plans"]["median_us_per_call"]
                                          / res["one_plan_of_T_targets"]["median_us_per_call"])
    if not grad:
        # (the envelope's time depends on the target: a single output's lines give other hulls than "all")
        names = ("cross_us", "covariance_us", "envelope_us")
        res["stage_times"] = {
            "single_target_plans": [{s: p.time_stage(Xd, i, 50) * 1e3 for i, s in enumerate(names)} for p in singles],
            "one_plan_of_T_targets": {s: joint.time_stage(Xd, i, 50) * 1e3 for i, s in enumerate(names)}}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", choices=sorted(CASES), help="run this case in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "targets", "bench_targets.json"))
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.reps, a.warmup)
    if a.reps < 30 or a.warmup < 5:
        print("note: fewer than 30 repeats / 5 warm-ups: not the documented measurement")
    res = {"timing": "wall time between device synchronisations, median of samples, legs alternated in one process",
           "reps": a.reps, "warmup": a.warmup}
    for name, case in CASES.items():
        # a fresh child per case, under its own time limit; a failure ends the run (nothing more is started)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=case[5])
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{name}: exit status {p.returncode}; stopping")
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        r = res[name]
        print(f"{name:18s} T={r['T']}: {r['single_target_plans']['median_us_per_call']:9.1f} us for T single-target "
              f"plans, {r['one_plan_of_T_targets']['median_us_per_call']:9.1f} us for one plan "
              f"(x{r['ratio_singles_over_one_plan']:.2f})", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
