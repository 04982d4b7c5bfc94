"""The posterior-mean Pareto front on the device against its numpy restatement.

``dkg_amd.pareto.sample_points_on_pareto_front`` on the golden ``lengthscales0`` surrogate (m = 2, d = 2, n = 100)
against ``tests/pareto_ref.run`` with the oracle's posterior mean on this box's host threads, timed in one process,
the legs alternated, synchronised wall time, median of the repeats after the warm-ups, at
  smoke      : 100 points x 100 generations   (the SMOKE_TEST shape, performance_after_scalarisation.py:14)
  production : 1000 points x 100 generations  (N_PARETO_POINTS = 1000)
The device leg is the whole call: the model's factorisation, the uniforms' draw and upload, the evolution, the
copies back.  ``device_evolution`` times ``dkg_pareto_nsga2`` alone on a prepared model (HIP launches to the final
synchronise).  It also records the front's quality ratio HV / H_grid (tests/golden/pareto_quality.json) of device
seeds 0-4 at the smoke shape.  ``device_evolution`` runs under the rank's selection rule (dkg_debug_pareto_wide
-1), ``device_evolution_one_workgroup`` under mode 0; ``grid_front`` is ``posterior_front_on_points`` on the
128 x 128 grid of the unit square (16384 points, always the wide rank).

``--rank-sweep`` times ``dkg_pareto_rank`` alone, the wide path (mode 1) against the one-workgroup kernel (mode 0),
legs alternated in one process: Q in {8 .. 2048}, keep = Q / 2, m in {2, 3, 8} (one per bucket), on a late-generation-like input
(60 % of the points on one front, so the peel is one round) and an early-generation-like one (uniform points, many
fronts).  A sample is the synchronised wall time of ``--inner`` calls enqueued back to back, per call, as the
evolution enqueues them.  The rule takes the wide path at a Q only where its median is below the one-workgroup
kernel's minimum on both inputs.

    python tools/bench_pareto.py                       # timings -> profiles/pareto_wide/bench_pareto.json
    python tools/bench_pareto.py --rank-sweep          # -> profiles/pareto_wide/rank_sweep.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_pareto.py --trace
    python tools/bench_pareto.py --kernel-stats DIR/.../run_kernel_stats.csv    # adds the stages' shares
(--trace-mode 0 traces the one-workgroup rank, --trace-grid the grid front; --stats-key names each merge)
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
from dkg_amd import _lib, pareto  # noqa: E402
from helpers import load_golden  # noqa: E402

SHAPES = {"smoke": (100, 100), "production": (1000, 100)}
RANK_WIDE = ("pareto_clear_kernel", "pareto_dom_kernel", "pareto_peel_kernel", "pareto_crowd_kernel",
             "pareto_order_kernel")
STAGES = {"posterior_mean": ("posterior_mean_kernel",), "rank": ("pareto_rank_kernel",) + RANK_WIDE,
          "variation": ("pareto_variation_kernel",),
          "glue": ("pareto_init_kernel", "pareto_gather_kernel")}
BOUNDS = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.double)
OUT_DIR = os.path.join(REPO, "profiles", "pareto_wide")
SWEEP_Q = (8, 16, 32, 64, 128, 200, 256, 512, 1024, 2000, 2048)


def with_mode(mode, fn):
    """fn() under dkg_debug_pareto_wide(mode); the previous mode is restored."""
    lib = _lib.load()
    prev = lib.dkg_debug_pareto_wide(mode)
    try:
        return fn()
    finally:
        lib.dkg_debug_pareto_wide(prev)


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


def measure(name, state, om, reps, warmup, numpy_leg=True):
    P, gens = SHAPES[name]
    dev = torch.device("cuda", 0)
    fit = pareto_ref.oracle_fitness(om, np.zeros(2), np.ones(2))
    u = pareto_ref.uniforms(0, P, 2, gens)
    pm = pareto.PreparedModel(state, dev)
    ud = torch.from_numpy(u).to(dev)
    legs = {"device": lambda: pareto.sample_points_on_pareto_front(state, BOUNDS, npoints=P, gen=gens, seed=0,
                                                                   device=dev),
            "device_evolution": lambda: pareto.pareto_nsga2(pm, BOUNDS[0], BOUNDS[1], P, gens, ud),
            "device_evolution_one_workgroup": lambda: with_mode(
                0, lambda: pareto.pareto_nsga2(pm, BOUNDS[0], BOUNDS[1], P, gens, ud)),
            "numpy": lambda: pareto_ref.run(fit, np.zeros(2), np.ones(2), P, gens, u, **pareto_ref.DEFAULTS)}
    if not numpy_leg:
        del legs["numpy"]
    res = alternate(legs, reps, warmup)
    res.update(P=P, generations=gens)
    if numpy_leg:
        res["ratio_numpy_over_device"] = res["numpy"]["median_ms"] / res["device"]["median_ms"]
    print(f"{name:10s} device {res['device']['median_ms']:9.2f} ms (evolution alone "
          f"{res['device_evolution']['median_ms']:8.2f} ms, one workgroup "
          f"{res['device_evolution_one_workgroup']['median_ms']:8.2f} ms)"
          + (f", numpy {res['numpy']['median_ms']:10.1f} ms" if numpy_leg else ""), flush=True)
    return res


def sweep_input(kind, Q, m, seed=0):
    """late: 60 % of the points on the plane sum f = 1 (mutually non-dominated), the others 0.9 of one of them
    (dominated), shuffled; early: uniform points of the unit cube."""
    g = np.random.default_rng(seed + 7 * Q + m)
    if kind == "early":
        return g.random((Q, m))
    nf = max(1, (6 * Q) // 10)
    front = g.dirichlet(np.ones(m), size=nf)
    rest = 0.9 * front[g.integers(0, nf, size=Q - nf)]
    return g.permutation(np.concatenate([front, rest]))


def rank_sweep(reps, warmup, inner):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for m in (2, 3, 8):  # one per objective bucket (2, 4, 8)
        for Q in SWEEP_Q:
            row = {"Q": Q, "m": m, "keep": Q // 2}
            for kind in ("late", "early"):
                F = torch.from_numpy(sweep_input(kind, Q, m)).to(dev)
                rank = torch.empty(Q, dtype=torch.int32, device=dev)
                crowd = torch.empty(Q, dtype=torch.double, device=dev)
                order = torch.empty(Q, dtype=torch.int32, device=dev)
                nbytes = int(lib.dkg_pareto_rank_workspace(Q, m))
                work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

                def calls():
                    for _ in range(inner):
                        _lib.check(lib.dkg_pareto_rank(F.data_ptr(), Q, m, Q // 2, rank.data_ptr(), crowd.data_ptr(),
                                                       order.data_ptr(), work.data_ptr(), nbytes, stream),
                                   "dkg_pareto_rank")

                legs = {"one_workgroup": lambda: with_mode(0, calls), "wide": lambda: with_mode(1, calls)}
                res = alternate(legs, reps, warmup)
                row[kind] = {k: {"median_us": v["median_ms"] * 1e3 / inner, "min_us": v["min_ms"] * 1e3 / inner}
                             for k, v in res.items()}
                row[kind]["fronts_ranked"] = int(rank.max().item()) + 1
            row["wide_wins"] = all(row[k]["wide"]["median_us"] < row[k]["one_workgroup"]["min_us"]
                                   for k in ("late", "early"))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return {"device": torch.cuda.get_device_name(0), "reps": reps, "warmup": warmup, "inner": inner,
            "timing": "synchronised wall time of `inner` calls enqueued back to back, per call; legs alternated",
            "rule": "wide where its median < the one-workgroup kernel's minimum on both inputs", "rows": rows}


def grid_front(state, reps, warmup):
    """posterior_front_on_points on the 128 x 128 grid of the unit square (Q = 16384): the whole call, the mean
    alone, and the rank alone (keep = 1)."""
    dev = torch.device("cuda", 0)
    pm = pareto.PreparedModel(state, dev)
    ax = np.linspace(0.0, 1.0, 128)
    G = torch.from_numpy(np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)).to(dev)
    f = pm.mean(G)
    legs = {"front_on_points": lambda: pareto.posterior_front_on_points(pm, G),
            "posterior_mean": lambda: pm.mean(G),
            "rank_keep_1": lambda: pareto.nondominated_rank(f, keep=1),
            "rank_keep_Q": lambda: pareto.nondominated_rank(f)}
    res = alternate(legs, reps, warmup)
    res.update(Q=int(G.shape[0]), front_points=int(pareto.posterior_front_on_points(pm, G)[0].shape[0]))
    print("grid front:", json.dumps(res), flush=True)
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


def trace(state, reps, mode, grid):
    """For a kernel trace: device evolutions of both shapes alone under dkg_debug_pareto_wide(mode), or (grid)
    posterior_front_on_points on the 128 x 128 grid alone."""
    dev = torch.device("cuda", 0)
    _lib.load().dkg_debug_pareto_wide(mode)
    pm = pareto.PreparedModel(state, dev)
    for P, gens in ({} if grid else SHAPES).values():
        ud = torch.from_numpy(pareto_ref.uniforms(0, P, 2, gens)).to(dev)
        for _ in range(reps):
            pareto.pareto_nsga2(pm, BOUNDS[0], BOUNDS[1], P, gens, ud)
    if grid:
        ax = np.linspace(0.0, 1.0, 128)
        G = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
        for _ in range(reps):
            pareto.posterior_front_on_points(pm, G)
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
    out = {k: {"total_us": tot[k], "calls": calls[k], "avg_us": tot[k] / max(calls[k], 1), "share": tot[k] / s}
           for k in STAGES}
    out["rank_kernels"] = {}
    for r in csv.DictReader(open(path)):
        if any(n in r["Name"] for n in STAGES["rank"]):
            out["rank_kernels"][r["Name"].split("(")[0][:60]] = {"calls": int(r["Calls"]),
                                                                 "avg_us": float(r["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big-reps", type=int, default=3, help="repeats at the production shape (the numpy leg is slow)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="default: profiles/pareto_wide/bench_pareto.json (rank_sweep.json)")
    ap.add_argument("--rank-sweep", action="store_true", help="dkg_pareto_rank alone, wide against one workgroup")
    ap.add_argument("--sweep-reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="calls enqueued back to back per sample of the sweep")
    ap.add_argument("--trace", action="store_true", help="run device evolutions only (for rocprofv3)")
    ap.add_argument("--trace-grid", action="store_true", help="with --trace: the 16384-point grid front alone")
    ap.add_argument("--trace-mode", type=int, default=-1, help="dkg_debug_pareto_wide mode of a --trace run")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a --trace run to merge into --out")
    ap.add_argument("--stats-key", default="stage_shares", help="the key --kernel-stats writes (one per traced mode)")
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy leg (minutes at the production shape)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(OUT_DIR, "rank_sweep.json" if a.rank_sweep else "bench_pareto.json")
    if a.kernel_stats:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res[a.stats_key] = kernel_stats(a.kernel_stats)
        print(json.dumps(res[a.stats_key], indent=1))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_pareto.py needs a ROCm device: there is no CPU timing of a GPU path")
        state, om, *_ = load_golden("lengthscales0")
        if a.trace:
            return trace(state, 3, a.trace_mode, a.trace_grid)
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res = {k: v for k, v in old.items() if k.startswith("stage_shares")}
        if a.rank_sweep:
            res = rank_sweep(a.sweep_reps, 5, a.inner)
        else:
            res.update(device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(),
                       timing="synchronised wall time, median, legs alternated", quality=quality(state))
            res["grid_front"] = grid_front(state, a.reps, a.warmup)
            res["smoke"] = measure("smoke", state, om, a.reps, a.warmup, not a.no_numpy)
            res["production"] = measure("production", state, om, a.big_reps, 1, not a.no_numpy)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
