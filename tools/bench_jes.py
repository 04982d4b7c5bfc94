"""Timing of the device joint entropy search at the reference preset's shape (bo_loop.py:142-159: 10 Pareto
samples x 10 points, batch_limit 50, raw_samples 512): m = 2, d = 2, n = 64 and 256 training points per output,
the boxes from the m = 2 staircase (compute_sample_box_decomposition).

Timed, synchronised wall time, median of --reps after --warmup, the legs alternated:
  forward_B50 / forward_B512   one forward of device candidates (no gradient)
  value_and_grad_host_B50      one value_and_grad_host call (host candidates in, [acq | dacq/dX] out)
  cpu_*                        the fp64 CPU restatement (tests/jes_oracle.py) on 16 threads, same shapes: the value
                               at B = 50 and B = 512, value + autograd gradient at B = 50 (--cpu-reps each)
for "LB" and "LB2" with all outputs observed, and "LB" observing output 0.  Nothing is asserted.

Per-kernel times come from a rocprofv3 run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_jes.py --trace
    python tools/bench_jes.py --kernel-stats DIR/.../run_kernel_stats.csv
--trace runs P in {3, 10} x m in {1, 2} models, 20 forwards with the gradient each, so that the trace shows an
evaluation to be two launches whatever P and m are (launches per evaluation = calls / 80 per kernel).

Writes profiles/jes/bench_jes.json.
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "decoupled-kg_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(REPO, "profiles", "jes", "bench_jes.json")


def problem(n, m=2, d=2, P=10, k=10, seed=0):
    """(state, pareto_sets, pareto_fronts, bounds): a grad_case model; per sample, k points spread over the
    non-dominated ones of the posterior mean on a pool of 512 uniform points (the first two objectives)."""
    from dkg_amd.jes import compute_sample_box_decomposition
    from helpers import grad_case, to_oracle

    state = grad_case(m, d, (n,), ("M52",), 4, 2, 1, seed)[0]
    om = to_oracle(state)
    g = torch.Generator().manual_seed(100 + seed)
    sets, fronts = [], []
    for _ in range(P):
        pool = torch.rand(512, d, generator=g, dtype=torch.double)
        with torch.no_grad():
            mean = torch.stack([o.posterior(pool)[0] for o in om.models], dim=1)
        m2 = mean[:, :2]
        dominated = ((m2[None] >= m2[:, None]).all(-1) & (m2[None] > m2[:, None]).any(-1)).any(1)
        nd = torch.nonzero(~dominated).reshape(-1)
        nd = nd[torch.argsort(m2[nd, 0])]
        pick = nd[torch.linspace(0, len(nd) - 1, min(k, len(nd))).round().long()].unique()
        sets.append(pool[pick])
        fronts.append(mean[pick] + 0.05 * torch.rand(len(pick), m, generator=g, dtype=torch.double))
    if m <= 2:
        bounds = compute_sample_box_decomposition(fronts)
    else:
        raise SystemExit("bench_jes builds boxes for m <= 2")
    return state, sets, fronts, bounds


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def alternate(legs, reps, warmup):
    """{name: median us} of the legs called in turn, reps times each after warmup rounds."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in times.items()}


def measure(n, est, target, reps, warmup, cpu_reps):
    import jes_oracle
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    state, sets, fronts, bounds = problem(n)
    acq = JES(state, sets, fronts, bounds, estimation_type=est, target_output_ix=target, device=DEV)
    g = torch.Generator().manual_seed(5)
    X50 = torch.rand(50, 1, 2, generator=g, dtype=torch.double)
    X512 = torch.rand(512, 1, 2, generator=g, dtype=torch.double)
    X50d, X512d = X50.to(DEV), X512.to(DEV)
    with torch.no_grad():
        res = alternate({"forward_B50": lambda: acq(X50d), "forward_B512": lambda: acq(X512d),
                         "value_and_grad_host_B50": lambda: acq.value_and_grad_host(X50)}, reps, warmup)
    ora = jes_oracle.OracleJES(state, sets, fronts, bounds, est, target)
    models, od = ora.models, ora.only_diagonal

    def cpu_value(X):
        with torch.no_grad():
            return jes_oracle.jes_value(models, ora.bounds, X.reshape(-1, 2), ora.target, od)

    def cpu_leg(fn):
        ts = []
        for _ in range(cpu_reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        return {"median_us": statistics.median(ts), "min_us": min(ts)}

    # the restatement takes its moments in chunks of jes_oracle.CHUNK candidates; the timing uses whole batches
    import functools
    orig = jes_oracle.moments
    try:
        jes_oracle.moments = functools.partial(orig, chunk=512)
        res["cpu_value_B50"] = cpu_leg(lambda: cpu_value(X50))
        res["cpu_value_B512"] = cpu_leg(lambda: cpu_value(X512))
        res["cpu_value_and_grad_B50"] = cpu_leg(
            lambda: jes_oracle.value_and_grad(models, ora.bounds, X50.reshape(-1, 2), ora.target, od))
    finally:
        jes_oracle.moments = orig
    with torch.no_grad():
        err = float((acq(X50) - cpu_value(X50)).abs().max())
    res["max_abs_diff_vs_cpu_B50"] = err
    res["boxes_J"] = int(bounds.shape[2])
    res["train_n_conditioned"] = [int(n + s.shape[0]) for s in sets]
    return res


def trace():
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    X = torch.rand(50, 2, dtype=torch.double)
    for P in (3, 10):
        for m in (1, 2):
            state, sets, fronts, bounds = problem(64, m=m, P=P)
            acq = JES(state, sets, fronts, bounds, device=DEV)
            for _ in range(20):
                acq.value_and_grad_host(X)
    torch.cuda.synchronize()
    print("done")


def kernel_stats(path):
    out = {}
    for r in csv.DictReader(open(path)):
        if "jes_" in r["Name"]:
            out[r["Name"].split("(")[0][:80]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    calls = {}
    for k, v in out.items():
        stage = "moments" if "moments" in k else "entropy"
        calls[stage] = calls.get(stage, 0) + v["calls"]
    return {"kernels": out, "calls_per_stage": calls, "evaluations": 80,
            "launches_per_evaluation": sum(calls.values()) / 80.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", action="store_true", help="device evaluations only (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a --trace run to merge into --out")
    a = ap.parse_args()
    torch.set_default_dtype(torch.double)
    if a.kernel_stats:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res["kernel_trace"] = kernel_stats(a.kernel_stats)
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["kernel_trace"], indent=1))
        return
    if a.trace:
        trace()
        return
    torch.set_num_threads(16)
    res = {"shape": "m=2 d=2 P=10 samples x 10 points, fp64; median of %d, legs alternated" % a.reps,
           "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads()}
    for n in (64, 256):
        for est, target in (("LB", None), ("LB2", None), ("LB", 0)):
            key = f"n{n}_{est}_t{'all' if target is None else target}"
            res[key] = measure(n, est, target, a.reps, a.warmup, a.cpu_reps)
            print(key, json.dumps(res[key]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
