"""The JES Pareto sampler on the device against its numpy restatement.

At the shape of the reference's ``jes_lb`` / ``jes_lb2`` presets (S = 10 samples, R = 512 features, population 100,
500 generations, target 10 points, m = 2, d = 2) on a synthetic model of n = 64 and n = 256 training points per
output, timed in one process, the legs alternated, synchronised wall time, median of the repeats after the warm-ups:

  sampler            ``sample_discrete_pareto_optimal_points``: draws, upload, weights, evolution, pruning, copies
  weights            ``dkg_rff_weights`` alone on uploaded draws (MFMA Gram tiles, the default)
  weights_valu       the same with the VALU Gram tiles (``dkg_debug_rff_gram(1)``)
  evolution_batched  ``dkg_pareto_nsga2_paths`` on the S paths
  evolution_serial   S calls of it with S = 1, one after the other
  restatement        tests/rff_ref.py: weights, evolution and pruning of ``--ref-samples`` samples for ``--ref-gens``
                     generations on this box's host threads, scaled to S samples and the preset's generations
                     (the restatement's cost is linear in both)

    python tools/bench_jes_pareto.py            # -> profiles/jes_pareto/bench.json
"""

import argparse
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
import rff_ref  # noqa: E402
from dkg_amd import _lib, jes_pareto  # noqa: E402
from helpers import grad_case  # noqa: E402

OUT_DIR = os.path.join(REPO, "profiles", "jes_pareto")
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": len(v)}
            for k, v in times.items()}


def with_gram(mode, fn):
    lib = _lib.load()
    prev = lib.dkg_debug_rff_gram(mode)
    try:
        return fn()
    finally:
        lib.dkg_debug_rff_gram(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--rffs", type=int, default=512)
    ap.add_argument("--pop", type=int, default=100)
    ap.add_argument("--gens", type=int, default=500)
    ap.add_argument("--target", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-samples", type=int, default=1)
    ap.add_argument("--ref-gens", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "bench.json"))
    a = ap.parse_args()
    torch.set_num_threads(16)
    dev = "cuda:0"
    S, R, P, gens, d, m = a.samples, a.rffs, a.pop, a.gens, 2, 2
    res = {"shape": dict(S=S, R=R, P=P, gens=gens, target=a.target, m=m, d=d), "device": torch.cuda.get_device_name(0),
           "n": {}}
    for n in (64, 256):
        state = grad_case(m, d, (n,), ("M52",), 4, 2, 4, 40 + n)[0]
        nus = [float(st.nu) for st in state.models]
        draws = jes_pareto.draw_rff_randomness(torch.Generator().manual_seed(1), nus, S, R, d)
        ddev = [t.to(dev) for t in draws]
        paths = jes_pareto.rff_weights(state, *ddev, device=dev)
        u = torch.rand(S, P * d + gens * pareto_ref.draws(P, d), dtype=torch.double,
                       generator=torch.Generator().manual_seed(2)).to(dev)
        singles = [(paths.sample(s), u[s:s + 1].contiguous()) for s in range(S)]
        legs = {
            "sampler": lambda: jes_pareto.sample_discrete_pareto_optimal_points(
                state, BOUNDS, S, a.target, num_rffs=R, nsga2_pop_size=P, nsga2_generations=gens, seed=0, device=dev),
            "weights": lambda: jes_pareto.rff_weights(state, *ddev, device=dev),
            "weights_valu": lambda: with_gram(1, lambda: jes_pareto.rff_weights(state, *ddev, device=dev)),
            "evolution_batched": lambda: jes_pareto.pareto_nsga2_paths(paths, BOUNDS[0], BOUNDS[1], P, gens, u),
            "evolution_serial": lambda: [jes_pareto.pareto_nsga2_paths(p1, BOUNDS[0], BOUNDS[1], P, gens, u1)
                                         for p1, u1 in singles],
        }
        out = alternate(legs, a.reps, a.warmup)
        # the restatement: a.ref_samples samples for a.ref_gens generations, scaled
        rs, rg = a.ref_samples, a.ref_gens
        sub = [t[:rs] for t in draws]
        un = u[:rs].cpu().numpy()
        prm = dict(cr=jes_pareto.SBX_PROB, eta_c=jes_pareto.SBX_ETA, m=min(0.5, 1.0 / d), eta_m=jes_pareto.PM_ETA)
        t0 = time.perf_counter()
        ref = rff_ref.weights(state, *sub)
        t1 = time.perf_counter()
        for s in range(rs):
            X, F, rank, _ = rff_ref.run(ref, s, np.zeros(d), np.ones(d), P, rg, un[s], **prm)
            rff_ref.prune(F, rank, a.target)
        t2 = time.perf_counter()
        w_ms, e_ms = (t1 - t0) * 1e3 * S / rs, (t2 - t1) * 1e3 * S / rs * gens / max(rg, 1)
        out["restatement"] = {"weights_ms_scaled": w_ms, "evolution_ms_scaled": e_ms, "total_ms_scaled": w_ms + e_ms,
                              "measured_samples": rs, "measured_gens": rg, "threads": torch.get_num_threads()}
        res["n"][str(n)] = out
        print(n, json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
