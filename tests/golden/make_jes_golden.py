"""Regenerates tests/golden/jes_entropy.npz: inputs and outputs of the reference's own entropy bound.

    python tests/golden/make_jes_golden.py /path/to/reference

The function ``_compute_entropy_upper_bound`` is taken out of the reference's
``src/decoupledbo/modules/acquisition/joint_entropy_search.py`` by ``ast`` when this script runs (it depends on
torch alone, so the BoTorch imports of its module are never executed) and evaluated on the CPU in fp64.  This
script holds none of the reference's text and the .npz holds numbers only; the tests read the .npz.

Cases: m in {1, 2, 3, 8} outputs x J in {1, 7, 70} boxes, P = 3 samples, B = 5 candidates; every case is
evaluated for only_diagonal in {False, True} (LB, LB2) and target_output_ix in {None, 0, m - 1}.  The boxes
of a sample are disjoint: a staircase in the first two objectives (intervals for m = 1) with lower bounds at
-1e10, and (-1e10, c_i] in the others; sample 1 keeps ceil(J / 2) boxes and is padded with [0, 0] boxes, as
the reference pads (jes_sample_pareto.py:243-245).  Condition on the inputs: every (candidate, sample) has
W = sum_j W_j >= 1e-3 (below that the reference's own Phi differences lose their digits); the seed of a case
is moved until the reference-side W satisfies it.
"""

import ast
import math
import os
import sys
from typing import Optional

import numpy as np
import torch
from torch import Tensor
from torch.distributions import Normal

HERE = os.path.dirname(os.path.abspath(__file__))
NEG = -1e10
P, B = 3, 5
MS = (1, 2, 3, 8)
JS = (1, 7, 70)
W_MIN = 1e-3
EPS = 2.0 ** -52


def reference_function(ref_root: str):
    path = os.path.join(ref_root, "src", "decoupledbo", "modules", "acquisition", "joint_entropy_search.py")
    with open(path) as fh:
        tree = ast.parse(fh.read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_compute_entropy_upper_bound")
    ns = {"torch": torch, "Normal": Normal, "pi": math.pi, "Tensor": Tensor, "Optional": Optional}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["_compute_entropy_upper_bound"]


def boxes(m: int, J: int, g: torch.Generator) -> Tensor:
    """[2, J, m] disjoint boxes of the dominated region of a staircase (intervals when m = 1)."""
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.double)  # noqa: E731
    a = torch.cumsum(0.05 + 2.0 * rnd(J) / J, 0) - 0.5            # increasing in the first objective
    lo = torch.full((J, m), NEG, dtype=torch.double)
    hi = torch.empty(J, m, dtype=torch.double)
    lo[1:, 0] = a[:-1]
    hi[:, 0] = a
    if m >= 2:
        hi[:, 1] = (torch.cumsum(0.05 + 2.0 * rnd(J) / J, 0) - 0.5).flip(0)   # decreasing in the second
    if m >= 3:
        hi[:, 2:] = 0.8 + rnd(m - 2)
    return torch.stack([lo, hi])


def case_inputs(m: int, J: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.double)  # noqa: E731
    bounds = torch.zeros(P, 2, J, m, dtype=torch.double)
    for p in range(P):
        Jp = (J + 1) // 2 if p == 1 else J    # sample 1: fewer boxes, the rest [0, 0] padding
        bounds[p, :, :Jp] = boxes(m, Jp, g)
    mean = 0.6 * rnd(B, P, m) - 0.1
    variance = 0.02 + 0.5 * rnd(B, P, m)
    noise = 1e-4 + 0.05 * rnd(B, P, m)
    return bounds, mean, variance, noise


def w_sum(bounds, mean, variance) -> Tensor:
    """sum_j W_j [B, P] with torch's Phi (the condition on the inputs)."""
    sd = variance.sqrt()[:, :, None]
    cdf = lambda z: 0.5 * (1 + torch.erf(z / math.sqrt(2.0)))  # noqa: E731
    gl = (bounds[None, :, 0] - mean[:, :, None]) / sd
    gu = (bounds[None, :, 1] - mean[:, :, None]) / sd
    return torch.exp(torch.log((cdf(gu) - cdf(gl)).clamp_min(EPS)).sum(-1)).sum(-1)


def main(ref_root: str) -> None:
    fn = reference_function(ref_root)
    out = {}
    for m in MS:
        for J in JS:
            seed = 1000 * m + J
            while True:
                bounds, mean, variance, noise = case_inputs(m, J, seed)
                if float(w_sum(bounds, mean, variance).min()) >= W_MIN:
                    break
                seed += 100000
            key = f"m{m}_J{J}"
            out[key + "_seed"] = np.array(seed)
            out[key + "_bounds"] = bounds.numpy()
            out[key + "_mean"] = mean.numpy()
            out[key + "_variance"] = variance.numpy()
            out[key + "_noise"] = noise.numpy()
            shape5 = lambda t: t.reshape(B, P, 1, 1, m)  # noqa: E731  batch x samples x q x 1 x M
            for diag in (False, True):
                for target in sorted({None, 0, m - 1}, key=lambda t: -1 if t is None else t):
                    h = fn(hypercell_bounds=bounds, mean=shape5(mean), variance=shape5(variance),
                           observation_noise=shape5(noise), target_output_ix=target, only_diagonal=diag)
                    assert h.shape == (B, 1) and bool(torch.isfinite(h).all()), (key, diag, target)
                    tname = "all" if target is None else str(target)
                    out[f"{key}_{'LB2' if diag else 'LB'}_t{tname}"] = h.reshape(B).numpy()
    np.savez_compressed(os.path.join(HERE, "jes_entropy.npz"), **out)
    print(f"wrote jes_entropy.npz: {len(out)} arrays")


if __name__ == "__main__":
    main(sys.argv[1])
