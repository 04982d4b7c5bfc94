"""The MAP fit's objective on the device against the host route.

Per objective evaluation (loss and gradient of fit_map's objective at its starting point) and per whole fit_map,
the device route (fit_map(device=...): one dkg_mll_value_grad call per evaluation) against the host route
(device=None: torch autograd on the CPU, this box's threads), timed in one process, alternating the legs,
synchronised wall time, median of --reps repeats after --warmup warm-ups, at
  once     : m = 2, n = 1000, d = 2   (bo_loop.fit_hyperparameters' 1000 Sobol points)
  always64 : m = 2, n = 64,   d = 2   (a refit inside the loop)
  always10 : m = 2, n = 10,   d = 2

    python tools/bench_fit.py                          # timings -> profiles/fit/bench_fit.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_fit.py --trace
    python tools/bench_fit.py --kernel-stats DIR/.../run_kernel_stats.csv     # adds the per-kernel times

mll_grad_kernel's counted work at n = 1000: the MFMAs it issues (one v_mfma_f64_16x16x4_f64 = 2048 flops; the
k-loop of tile row ti runs over the rows 32 ti .. n in steps of 32), against the 78.6 TF fp64 matrix roof, and
the n (n + 1) / 2 pair evaluations of its epilogue (kappa, h, d squares each).
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dkg_amd import fit  # noqa: E402
from dkg_amd.bo_smoke import reference_model_config  # noqa: E402

FP64_MATRIX_TF = 78.6
SHAPES = {"once": (2, 1000, 2, "once"), "always64": (2, 64, 2, "always"), "always10": (2, 10, 2, "always")}
KERNELS = ("mll_grad_kernel", "mll_finalize_kernel", "chol_step_kernel", "chol_finalize_kernel", "trinv_col_kernel",
           "alpha_kernel", "kernel_matrix_kernel")


def problem(name):
    m, n, d, mode = SHAPES[name]
    g = torch.Generator().manual_seed(7)
    X = torch.quasirandom.SobolEngine(d, scramble=True, seed=7).draw(n, dtype=torch.double)
    ls = torch.tensor([0.15, 0.5], dtype=torch.double)[:d]
    t = 5.0 ** 0.5 * torch.cdist(X / ls, X / ls)
    K = 2.0 * (1 + t + t * t / 3) * torch.exp(-t) + 1e-4 * torch.eye(n, dtype=torch.double)
    L = torch.linalg.cholesky(K)
    ys = [0.3 + L @ torch.randn(n, generator=g, dtype=torch.double) for _ in range(m)]
    return [X] * m, ys, reference_model_config(m, [[0.0] * d, [1.0] * d], mode)


def objectives(xs, ys, cfg, dev):
    """fit_map's two objectives over the same outputs, and its starting point."""
    outs = [fit._Output(xs[i], ys[i], cfg["outputs"][i], fit.MIN_NOISE_SE, None) for i in range(len(xs))]
    x0 = np.array([v for o in outs for v in o.initial()], dtype=np.float64)

    def host(v):
        raw = torch.tensor(v, dtype=torch.double, requires_grad=True)
        k, loss = 0, 0.0
        for o in outs:
            loss = loss - o.mll(raw[k:k + o.n_raw])
            k += o.n_raw
        (g,) = torch.autograd.grad(loss, raw)
        return float(loss.detach()), g.numpy().astype(np.float64)

    return host, fit._device_objective(outs, dev), x0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(legs, reps, warmup):
    times = {k: [] for k in legs}
    last = {}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t, last[k] = timed(fn)
            if r >= warmup:
                times[k].append(t)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "reps": len(v)} for k, v in times.items()}, last


def mfma_flops(n):
    nt = (n + 31) // 32
    per_wave = sum((ti + 1) * (-(-(n - 32 * ti) // 32) * 8) for ti in range(nt))  # MFMAs of one sub-tile per tile row
    return 4 * per_wave * 2048


def measure(name, reps, warmup, fit_reps):
    xs, ys, cfg = problem(name)
    dev = torch.device("cuda", 0)
    host, device, x0 = objectives(xs, ys, cfg, dev)
    ev, last = alternate({"host": lambda: host(x0), "device": lambda: device(x0)}, reps, warmup)
    gap = float(np.abs(last["host"][1] - last["device"][1]).max() / np.abs(last["host"][1]).max())
    ft, fl = alternate({"host": lambda: fit.fit_map(xs, ys, cfg),
                        "device": lambda: fit.fit_map(xs, ys, cfg, device=dev)}, fit_reps, 1)
    m, n, d, _ = SHAPES[name]
    res = {"m": m, "n": n, "d": d, "evaluation": ev, "evaluation_gradient_gap": gap, "fit_map": ft,
           "evaluation_ratio_host_over_device": ev["host"]["median_ms"] / ev["device"]["median_ms"],
           "fit_ratio_host_over_device": ft["host"]["median_ms"] / ft["device"]["median_ms"],
           "fit_iterations": {k: v["iterations"] for k, v in fl.items()},
           "fit_mll": {k: v["mll"] for k, v in fl.items()}}
    print(f"{name:9s} evaluation: host {ev['host']['median_ms']:9.3f} ms, device {ev['device']['median_ms']:8.3f} ms "
          f"(gradient gap {gap:.1e}); fit_map: host {ft['host']['median_ms']:10.1f} ms, device "
          f"{ft['device']['median_ms']:9.1f} ms, iterations {res['fit_iterations']}", flush=True)
    return res


def trace(reps):
    """Device evaluations of the `once` shape alone, for a kernel trace."""
    xs, ys, cfg = problem("once")
    _, device, x0 = objectives(xs, ys, cfg, torch.device("cuda", 0))
    for _ in range(reps):
        device(x0)
    torch.cuda.synchronize()
    print("done")


def kernel_stats(path):
    """Average time per kernel of a device evaluation from a rocprofv3 kernel-stats CSV of a --trace run."""
    m, n, d, _ = SHAPES["once"]
    out = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Name"]:
                out[k] = {"avg_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"]),
                          "total_us": float(r["AverageNs"]) * int(r["Calls"]) / 1e3}
    if "mll_grad_kernel" in out:
        g = out["mll_grad_kernel"]
        flops = m * mfma_flops(n)  # one launch carries both outputs
        tf = flops / (g["avg_us"] * 1e-6) / 1e12
        total = sum(v["total_us"] for v in out.values())
        g.update(mfma_flops=flops, pairs=m * n * (n + 1) // 2, TFs=tf, of_fp64_matrix_roof=tf / FP64_MATRIX_TF,
                 share_of_kernel_time=g["total_us"] / total)
        out["kernel_time_us_per_evaluation"] = total / g["calls"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit", "bench_fit.json"))
    ap.add_argument("--trace", action="store_true",
                    help="run device evaluations of the once shape only (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a --trace run to merge into --out")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res["kernels_once"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["kernels_once"], indent=1))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_fit.py needs a ROCm device: there is no CPU timing of a GPU path")
        if a.trace:
            return trace(max(a.reps, 20))
        if a.reps < 30 or a.warmup < 5:
            print("note: fewer than 30 repeats / 5 warm-ups: not the documented measurement")
        keep = json.load(open(a.out)).get("kernels_once") if os.path.exists(a.out) else None
        res = {"kernels_once": keep} if keep else {}
        res.update(device=torch.cuda.get_device_name(0), timing="synchronised wall time, median, legs alternated",
                   host_threads=torch.get_num_threads(), fp64_matrix_roof_TFs=FP64_MATRIX_TF)
        for name in SHAPES:
            res[name] = measure(name, a.reps, a.warmup, a.fit_reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
