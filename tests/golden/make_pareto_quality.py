"""Generates tests/golden/pareto_quality.json: the quality yardstick of the device NSGA-II front
(tests/test_gpu_pareto.py), computed on the CPU from the numpy restatement (tests/pareto_ref.py) and the oracle.

On the ``lengthscales0`` golden surrogate (m = 2, d = 2, unit-cube bounds):

* H_grid: the hypervolume, above the fixture's ``ref_point`` (tests/golden/shared/gp-problem/lengthscales/0.pt, the
  reference's shared problem file), of the oracle mean on a 129 x 129 grid of the unit square (the dominated points
  of the grid add nothing to it);
* for seeds 0-4 the restatement runs P = 100, gen = GEN; r_s = HV(rank-0 front of the final population) / H_grid
  and r0_s the same ratio at generation 0;
* t = r_min - 2 (r_max - r_min): the worst seed less twice the seed-to-seed spread (a device run can leave the CPU
  trajectory at a rounding-level tie, and is then one more draw from the same distribution).

The generator checks that every r0_s < t (otherwise the test could not tell evolution from the initial sample).

Run from the repository root: python tests/golden/make_pareto_quality.py
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "decoupled-kg_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pareto_ref  # noqa: E402
from helpers import load_golden  # noqa: E402

P, GEN, SEEDS, GRID = 100, 100, (0, 1, 2, 3, 4), 129


def main():
    om = load_golden("lengthscales0")[1]
    ax = np.linspace(0.0, 1.0, GRID)
    G = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    FG = pareto_ref.oracle_mean(om, G)
    shared = torch.load(os.path.join(HERE, "shared", "gp-problem", "lengthscales", "0.pt"), weights_only=True)
    ref = np.asarray(shared["ref_point"], dtype=np.float64)
    H = pareto_ref.hypervolume_2d(FG, ref)
    lb, ub = np.zeros(2), np.ones(2)
    fit = pareto_ref.oracle_fitness(om, lb, ub)
    r, r0 = [], []
    for s in SEEDS:
        hist = []
        pareto_ref.run(fit, lb, ub, P, GEN, pareto_ref.uniforms(s, P, 2, GEN), history=hist, **pareto_ref.DEFAULTS)
        for (X, F, rank), out in ((hist[0], r0), (hist[-1], r)):
            out.append(pareto_ref.hypervolume_2d(F[rank == 0], ref) / H)
        print(f"seed {s}: r0 = {r0[-1]:.6f}  r = {r[-1]:.6f}", flush=True)
    t = min(r) - 2.0 * (max(r) - min(r))
    assert all(v < t for v in r0), (r0, t)
    out = {"problem": "lengthscales0", "P": P, "gen": GEN, "grid": GRID, "seeds": list(SEEDS),
           "ref_point": ref.tolist(), "H_grid": H, "r": r, "r0": r0, "t": t}
    with open(os.path.join(HERE, "pareto_quality.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
