"""The weight-posterior cases of the JES Pareto sampler's tests: test infrastructure shared by
tests/test_jes_pareto_host.py (which asserts the rounding-floor condition on every case) and
tests/test_gpu_jes_pareto.py (which asserts the device against the restatement on the same cases)."""

import functools
import math

import numpy as np
import torch

import rff_ref
from dkg_amd.jes_pareto import draw_rff_randomness
from dkg_amd.model import ModelListGPState, SingleTaskGPState
from helpers import FAMILIES

# id -> ns (one per output), R, d, families, Standardize, noise, outputscale, lengthscale, S
WEIGHT_CASES = {
    "n10-R64-d1-m1": dict(ns=(10,), R=64, d=1, fam=("M52",), std=True, noise=1e-2, s=1.0, ls=0.3, S=2),
    "n40-R100-d2-m2": dict(ns=(40, 40), R=100, d=2, fam=("M32", "RBF"), std=True, noise=1e-2, s=2.0, ls=0.4, S=2),
    "n127-R512-d6-m3": dict(ns=(127, 127, 127), R=512, d=6, fam=("M12", "M52", "RBF"), std=False, noise=1e-2, s=1.5,
                            ls=0.8, S=2),
    "n40-R64-d16-m2": dict(ns=(40, 40), R=64, d=16, fam=("RBF", "M12"), std=True, noise=1e-2, s=1.0, ls=1.5, S=2),
    "n127-R1024-d2-m1": dict(ns=(127,), R=1024, d=2, fam=("M32",), std=False, noise=1e-2, s=1.0, ls=0.3, S=1),
    "n10-R100-d6-m3": dict(ns=(10, 10, 10), R=100, d=6, fam=("M52", "M32", "M12"), std=True, noise=1e-2, s=1.0,
                           ls=0.9, S=2),
    # nine problems: two batches of the factorisation, outputs of different n
    "mixed-R512-d2-m3-S3": dict(ns=(10, 40, 127), R=512, d=2, fam=("M52", "M32", "RBF"), std=True, noise=1e-2, s=1.0,
                                ls=0.3, S=3),
    # the issue's harder floor: noise 1e-4 at s = 50, l = 0.2
    "n40-R512-d2-m2-noise1e-4": dict(ns=(40, 40), R=512, d=2, fam=("M52", "RBF"), std=True, noise=1e-4, s=50.0,
                                     ls=0.2, S=2),
}


def make_state(ns, d, fam, std, noise, s, ls, seed):
    g = torch.Generator().manual_seed(int(seed))
    models = []
    for i, n in enumerate(ns):
        x = torch.rand(n, d, generator=g, dtype=torch.double)
        y = torch.sin(3.0 * x.sum(-1) / math.sqrt(d) + i) + 0.1 * torch.randn(n, generator=g, dtype=torch.double)
        lsv = ls * (0.75 + 0.5 * torch.rand(d, generator=g, dtype=torch.double))
        kind, nu = FAMILIES[fam[i % len(fam)]]
        models.append(SingleTaskGPState(x, y, lsv, s * (1.0 + 0.25 * i), noise * (1 + i), 0.1 * i - 0.2, kind,
                                        2.5 if nu is None else nu, 0.3 * i + 0.5 if std else 0.0,
                                        1.0 + 0.25 * i if std else 1.0))
    return ModelListGPState(*models)


@functools.lru_cache(maxsize=None)
def weight_case(name):
    """-> (state, draws (wn, g, ub, z), eval points [64 + sum n, d], restatement paths, spread [S, m]): the spread is
    the largest difference, over the points, between the restatement's paths with the training rows as given and
    reversed -- the reference side's own rounding floor."""
    kw = WEIGHT_CASES[name]
    seed = sorted(WEIGHT_CASES).index(name) + 1
    state = make_state(kw["ns"], kw["d"], kw["fam"], kw["std"], kw["noise"], kw["s"], kw["ls"], seed)
    nus = [None if st.kernel == "rbf" else float(st.nu) for st in state.models]
    draws = draw_rff_randomness(torch.Generator().manual_seed(100 + seed), nus, kw["S"], kw["R"], kw["d"])
    sobol = torch.quasirandom.SobolEngine(kw["d"], scramble=False).draw(64).to(torch.double)
    pts = torch.cat([sobol] + [st.train_x for st in state.models]).numpy()
    ref = rff_ref.weights(state, *draws)
    rev = rff_ref.weights(state, *draws, reverse_rows=True)
    spread = np.abs(rff_ref.evaluate(ref, pts) - rff_ref.evaluate(rev, pts)).max(1)
    return state, draws, pts, ref, spread


def spread_cap(state):
    """[m]: the condition every asserted case meets: spread <= 1e-6 y_std sqrt(s)."""
    return np.array([1e-6 * float(st.y_std) * math.sqrt(float(st.outputscale)) for st in state.models])
