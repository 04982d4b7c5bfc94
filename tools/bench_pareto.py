"""The posterior-mean Pareto front on the device against its numpy restatement.

``dkg_amd.pareto.sample_points_on_pareto_front`` on the golden ``lengthscales0`` surrogate (m = 2, d = 2, n = 100)
against ``tests/pareto_ref.run`` with the oracle's posterior mean on this box's host threads, timed in one process,
the legs alternated, synchronised wall time, median of the repeats after the warm-ups, at
  smoke      : 100 points x 100 generations   (the SMOKE_TEST shape, performance_after_scalarisation.py:14)
  production : 1000 points x 100 generations  (N_PARETO_POINTS = 1000)
The device leg is the whole call: the model's factorisation, the uniforms' draw and upload, the evolution, the
copies back.  ``device_evolution`` times ``dkg_pareto_nsga2`` alone on a prepared model (HIP launches to the final
synchronise).  It also records the front's quality ratio HV / H_grid (tests/golden/pareto_quality.json) of device
seeds 0-4 at the smoke shape.

    python tools/bench_pareto.py                       # timings -> profiles/pareto/bench_pareto.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_pareto.py --trace
    python tools/bench_pareto.py --kernel-stats DIR/.../run_kernel_stats.csv    # adds the stages' shares
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pareto_ref  # noqa: E402
from dkg_amd import pareto  # noqa: E402
from helpers import load_golden  # noqa: E402

SHAPES = {"smoke": (100, 100), "production": (1000, 100)}
STAGES = {"posterior_mean": ("posterior_mean_kernel",), "rank": ("pareto_rank_kernel",),
          "variation": ("pareto_variation_kernel",),
          "glue": ("pareto_init_kernel", "pareto_normalise_kernel", "pareto_gather_kernel")}
BOUNDS = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.double)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(legs, reps, warmup):
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t, _ = timed(fn)
            if r >= warmup:
                times[k].append(t)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "reps": len(v)} for k, v in times.items()}


def measure(name, state, om, reps, warmup):
    P, gens = SHAPES[name]
    dev = torch.device("cuda", 0)
    fit = pareto_ref.oracle_fitness(om, np.zeros(2), np.ones(2))
    u = pareto_ref.uniforms(0, P, 2, gens)
    pm = pareto.PreparedModel(state, dev)
    ud = torch.from_numpy(u).to(dev)
    legs = {"device": lambda: pareto.sample_points_on_pareto_front(state, BOUNDS, npoints=P, gen=gens, seed=0,
                                                                   device=dev),
            "device_evolution": lambda: pareto.pareto_nsga2(pm, BOUNDS[0], BOUNDS[1], P, gens, ud),
            "numpy": lambda: pareto_ref.run(fit, np.zeros(2), np.ones(2), P, gens, u, **pareto_ref.DEFAULTS)}
    res = alternate(legs, reps, warmup)
    res.update(P=P, generations=gens, ratio_numpy_over_device=res["numpy"]["median_ms"] / res["device"]["median_ms"])
    print(f"{name:10s} device {res['device']['median_ms']:9.2f} ms (evolution alone "
          f"{res['device_evolution']['median_ms']:8.2f} ms), numpy {res['numpy']['median_ms']:10.1f} ms", flush=True)
    return res


def quality(state):
    q = json.load(open(os.path.join(REPO, "tests", "golden", "pareto_quality.json")))
    out = []
    for s in q["seeds"]:
        _, f = pareto.sample_points_on_pareto_front(state, BOUNDS, npoints=q["P"], gen=q["gen"], seed=s,
                                                    device="cuda:0")
        out.append(pareto_ref.hypervolume_2d(f, q["ref_point"]) / q["H_grid"])
    print("device HV / H_grid, seeds 0-4:", out, " CPU:", q["r"], " t =", q["t"], flush=True)
    return {"device_ratio": out, "cpu_ratio": q["r"], "threshold": q["t"]}


def trace(state, reps):
    """Device evolutions of both shapes alone, for a kernel trace."""
    dev = torch.device("cuda", 0)
    pm = pareto.PreparedModel(state, dev)
    for P, gens in SHAPES.values():
        ud = torch.from_numpy(pareto_ref.uniforms(0, P, 2, gens)).to(dev)
        for _ in range(reps):
            pareto.pareto_nsga2(pm, BOUNDS[0], BOUNDS[1], P, gens, ud)
    torch.cuda.synchronize()
    print("done")


def kernel_stats(path):
    """Each stage's share of the kernel time of a --trace run (both shapes together; the production shape
    dominates), from a rocprofv3 kernel-stats CSV."""
    tot = {k: 0.0 for k in STAGES}
    calls = {k: 0 for k in STAGES}
    for r in csv.DictReader(open(path)):
        for k, names in STAGES.items():
            if any(n in r["Name"] for n in names):
                tot[k] += float(r["AverageNs"]) * int(r["Calls"]) / 1e3
                calls[k] += int(r["Calls"])
    s = sum(tot.values()) or 1.0
    return {k: {"total_us": tot[k], "calls": calls[k], "avg_us": tot[k] / max(calls[k], 1), "share": tot[k] / s}
            for k in STAGES}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big-reps", type=int, default=3, help="repeats at the production shape (the numpy leg is slow)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pareto", "bench_pareto.json"))
    ap.add_argument("--trace", action="store_true", help="run device evolutions only (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a --trace run to merge into --out")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res["stage_shares"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["stage_shares"], indent=1))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_pareto.py needs a ROCm device: there is no CPU timing of a GPU path")
        state, om, *_ = load_golden("lengthscales0")
        if a.trace:
            return trace(state, 3)
        keep = json.load(open(a.out)).get("stage_shares") if os.path.exists(a.out) else None
        res = {"stage_shares": keep} if keep else {}
        res.update(device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(),
                   timing="synchronised wall time, median, legs alternated", quality=quality(state))
        res["smoke"] = measure("smoke", state, om, a.reps, a.warmup)
        res["production"] = measure("production", state, om, a.big_reps, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
