"""Timing of the device hypervolume knowledge gradient at the reference preset's shape (bo_loop.py:122-160:
num_fantasies 32, num_pareto 10, batch_limit 5, raw_samples 512): m = 2, d = 2, n = 64 and 256 training points per
output, output 0 observed (one of the decoupled runs).

Timed, synchronised wall time, median of --reps after --warmup, the legs alternated:
  value_and_grad_host_B5   one value_and_grad_host call of 5 one-shot points (321 rows each; host in, host out)
  screen_B512              the no-gradient screen of 512 one-shot points (164 352 rows) resident on the device
  value_function_B20_q10   the value function with its gradient at 20 sets of 10 points (value_and_grad_host)
  cpu_*                    the fp64 CPU restatement (tests/hvkg_oracle.py) on 16 threads, same shapes
                           (--cpu-reps each; cpu_screen is timed on --cpu-screen points and scaled to 512)
Nothing is asserted.

Per-kernel times and the launch count come from a rocprofv3 run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_hvkg.py --trace
    python tools/bench_hvkg.py --kernel-stats DIR/.../run_kernel_stats.csv
--trace runs (Nf, Np, m, B) in {(32, 10, 2, 5), (3, 4, 3, 17), (1, 1, 2, 1)}, 20 value + gradient evaluations each,
and 20 of the value function, so that the trace shows an evaluation to be four launches (three for the value
function) whatever B, Nf, Np and m are.

Writes profiles/hvkg/bench.json.
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
OUT = os.path.join(REPO, "profiles", "hvkg", "bench.json")
NF, NP = 32, 10


def problem(n, m=2, d=2, Nf=NF, Np=NP, seed=0):
    """(state, ref, z): a grad_case model; ref a tenth of each objective's range below the smallest posterior mean
    over a pool of 512 uniform points."""
    from helpers import grad_case, to_oracle

    state = grad_case(m, d, (n,), ("M52",), 4, 2, 1, seed)[0]
    g = torch.Generator().manual_seed(100 + seed)
    pool = torch.rand(512, d, generator=g, dtype=torch.double)
    with torch.no_grad():
        mean = torch.stack([o.posterior(pool)[0] for o in to_oracle(state).models], dim=1)
    ref = mean.min(0).values - 0.1 * (mean.max(0).values - mean.min(0).values)
    z = torch.randn(Nf, m, generator=g, dtype=torch.double)
    return state, ref, z


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


def cpu_leg(fn, reps, scale=1.0):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6 * scale)
    return {"median_us": statistics.median(ts), "min_us": min(ts)}


def measure(n, reps, warmup, cpu_reps, cpu_screen):
    import hvkg_oracle as ho
    from dkg_amd.hvkg import PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient

    state, ref, z = problem(n)
    mask = torch.tensor([[True, False]])
    acq = qHypervolumeKnowledgeGradient(state, ref, num_fantasies=NF, num_pareto=NP, X_evaluation_mask=mask,
                                        current_value=0.5, cost_aware_utility=[1.0, 2.0], base_samples=z, device=DEV)
    vf = PosteriorMeanHypervolume(state, ref, device=DEV)
    g = torch.Generator().manual_seed(5)
    X5 = torch.rand(5, 1 + NF * NP, 2, generator=g, dtype=torch.double)
    X512d = torch.rand(512, 1 + NF * NP, 2, generator=g, dtype=torch.double).to(DEV)
    V20 = torch.rand(20, NP, 2, generator=g, dtype=torch.double)
    with torch.no_grad():
        res = alternate({"value_and_grad_host_B5": lambda: acq.value_and_grad_host(X5),
                         "screen_B512": lambda: acq(X512d),
                         "value_function_B20_q10": lambda: vf.value_and_grad_host(V20)}, reps, warmup)
    models = ho.models_of(state)

    def cpu_value_and_grad(X):
        Xr = X.clone().requires_grad_(True)
        a, _ = ho.acquisition(models, Xr, z, 1, NF, NP, ref, 0.5, 1.0)
        return a.detach(), torch.autograd.grad(a.sum(), Xr)[0]

    def cpu_screen_leg():
        with torch.no_grad():
            ho.acquisition(models, X512d[:cpu_screen].cpu(), z, 1, NF, NP, ref, 0.5, 1.0)

    def cpu_vf():
        Xr = V20.clone().requires_grad_(True)
        a, _ = ho.value_function(models, Xr, ref)
        torch.autograd.grad(a.sum(), Xr)

    res["cpu_value_and_grad_B5"] = cpu_leg(lambda: cpu_value_and_grad(X5), cpu_reps)
    res["cpu_screen_B512"] = cpu_leg(cpu_screen_leg, cpu_reps, 512.0 / cpu_screen)
    res["cpu_screen_B512"]["scaled_from_points"] = cpu_screen
    res["cpu_value_function_B20_q10"] = cpu_leg(cpu_vf, cpu_reps)
    val, grad = acq.value_and_grad_host(X5)
    cv, cg = cpu_value_and_grad(X5)
    res["max_abs_diff_vs_cpu_B5"] = {"value": float((val - cv).abs().max()), "gradient": float((grad - cg).abs().max())}
    return res


def trace():
    from dkg_amd.hvkg import PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient

    g = torch.Generator().manual_seed(5)
    for Nf, Np, m, B in ((32, 10, 2, 5), (3, 4, 3, 17), (1, 1, 2, 1)):
        state, ref, z = problem(64, m=m, Nf=Nf, Np=Np)
        acq = qHypervolumeKnowledgeGradient(state, ref, num_fantasies=Nf, num_pareto=Np, base_samples=z, device=DEV)
        X = torch.rand(B, 1 + Nf * Np, 2, generator=g, dtype=torch.double)
        for _ in range(20):
            acq.value_and_grad_host(X)
    vf = PosteriorMeanHypervolume(state, ref, device=DEV)
    V = torch.rand(20, NP, 2, generator=g, dtype=torch.double)
    for _ in range(20):
        vf.value_and_grad_host(V)
    torch.cuda.synchronize()
    print("done")


def kernel_stats(path):
    out, calls = {}, {}
    for r in csv.DictReader(open(path)):
        if "hvkg_" in r["Name"]:
            out[r["Name"].split("(")[0][:80]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    for k, v in out.items():
        stage = next(s for s in ("cand", "fantasy", "hv", "finish") if f"hvkg_{s}_kernel" in k)
        calls[stage] = calls.get(stage, 0) + v["calls"]
    return {"kernels": out, "calls_per_stage": calls, "one_shot_evaluations": 60, "value_function_evaluations": 20,
            "expected_launches": 60 * 4 + 20 * 3, "launches": sum(calls.values())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-screen", type=int, default=16, help="one-shot points the CPU screen leg is timed on")
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
    res = {"shape": "m=2 d=2 num_fantasies=32 num_pareto=10 (321 rows), output 0 observed, fp64; median of %d, legs "
                    "alternated" % a.reps,
           "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads()}
    for n in (64, 256):
        res[f"n{n}"] = measure(n, a.reps, a.warmup, a.cpu_reps, a.cpu_screen)
        print(f"n{n}", json.dumps(res[f"n{n}"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
