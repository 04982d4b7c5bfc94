"""Bit-identity of two builds of libdkg.so (DKG_LIB A/B): forward KG, KG per pair and the value+gradient
path on several workloads, then the acquisition layer (posterior mean, sample paths, NSGA-II, ranks, JES, HVKG,
boxes) at small ragged shapes in every dimension bucket and covariance family.

Run on the GPU box from the repo root:  python tools/ab_bits.py <libA.so> <libB.so> [--acq-only] [--json OUT]
Each build runs in its own subprocess under a time limit (the library is loaded once per process), the second
only after the first ended well; prints, per output, whether the two builds agree bit for bit, and with --json
writes the table.  --acq-only skips the KG workloads.
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = (("matern", 0.5), ("matern", 1.5), ("matern", 2.5), ("rbf", None))


def dump_acquisition(out):
    """Every entry of the acquisition layer where the shared pieces can go wrong: d < DM in each bucket (the
    clamped loads), n no multiple of 16 or 64, all four families, m = 2 and 3."""
    import torch

    from dkg_amd import _lib
    from dkg_amd.boxes import dominated_boxes, dominated_boxes_device, hypervolume_front_device
    from dkg_amd.hvkg import PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch
    from dkg_amd.jes_pareto import pareto_nsga2_paths, sample_rff_paths
    from dkg_amd.model import ModelListGPState, SingleTaskGPState
    from dkg_amd.pareto import PreparedModel, nondominated_rank, pareto_draws, pareto_nsga2

    lib = _lib.load()
    case = 0
    for d in (1, 3, 5, 9):
        for n in (37, 100):
            for fi, (kind, nu) in enumerate(FAMILIES):
                for m in (2, 3):
                    case += 1
                    g = torch.Generator().manual_seed(1000 + case)
                    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.double)  # noqa: E731
                    state = ModelListGPState(*[
                        SingleTaskGPState(rnd(n - i, d), torch.randn(n - i, generator=g, dtype=torch.double),
                                          0.3 + rnd(d), 0.8 + 0.1 * i, 1e-2, 0.1 * i, kind, 2.5 if nu is None else nu,
                                          0.2 * i, 1.0 + 0.5 * i) for i in range(m)])
                    key = f"acq/d{d}-n{n}-{kind}{'' if nu is None else nu}-m{m}"
                    pm = PreparedModel(state)
                    out[key + "/posterior_mean"] = pm.mean(rnd(19, d)).cpu()
                    paths = sample_rff_paths(state, 2, 70, seed=case)
                    out[key + "/rff_eval"] = paths(rnd(19, d)).cpu()
                    lb, ub, P, gens = torch.zeros(d), torch.ones(d), 8, 2
                    per = P * d + gens * pareto_draws(P, d)
                    for name, res in (("pareto_nsga2", pareto_nsga2(pm, lb, ub, P, gens, rnd(per))),
                                      ("nsga2_paths", pareto_nsga2_paths(paths, lb, ub, P, gens, rnd(2, per)))):
                        for part, t in zip(("X", "F", "rank", "crowd"), res):
                            out[f"{key}/{name}/{part}"] = t.cpu()
                    F = (rnd(70, m) * 8).floor() / 8  # ties
                    for mode in (0, 1):  # the one-workgroup rank, the wide rank
                        prev = lib.dkg_debug_pareto_wide(mode)
                        try:
                            for part, t in zip(("rank", "crowd", "order"), nondominated_rank(F.cuda(), keep=35)):
                                out[f"{key}/rank_mode{mode}/{part}"] = t.cpu()
                        finally:
                            lib.dkg_debug_pareto_wide(prev)
                    sets = [rnd(3, d) for _ in range(2)]
                    fronts = [torch.randn(3, m, generator=g, dtype=torch.double) for _ in range(2)]
                    jes = qLowerBoundMultiObjectiveJointEntropySearch(state, sets, fronts, dominated_boxes(fronts),
                                                                      estimation_type="LB" if fi % 2 else "LB2")
                    Xj = rnd(17, 1, d).cuda().requires_grad_(True)
                    vj = jes(Xj)
                    out[key + "/jes/value"] = vj.detach().cpu()
                    out[key + "/jes/grad"] = torch.autograd.grad(vj.sum(), Xj)[0].cpu()
                    ref = [-10.0] * m
                    mask = torch.tensor([[True] + [False] * (m - 2) + [True]]) if m == 3 else torch.tensor([[False, True]])
                    hv = qHypervolumeKnowledgeGradient(state, ref, num_fantasies=3, num_pareto=4, X_evaluation_mask=mask,
                                                       current_value=0.5, seed=case)
                    Xh = rnd(3, 13, d).cuda().requires_grad_(True)
                    vh = hv(Xh)
                    out[key + "/hvkg/value"] = vh.detach().cpu()
                    out[key + "/hvkg/grad"] = torch.autograd.grad(vh.sum(), Xh)[0].cpu()
                    out[key + "/hvkg/value_function"] = PosteriorMeanHypervolume(state, ref)(rnd(3, 5, d).cuda()).cpu()
    g = torch.Generator().manual_seed(7)
    for m in (1, 2, 3):
        Y = ((torch.rand(3, 70, m, generator=g, dtype=torch.double) * 16).floor() / 16).cuda()
        ref = [0.125] * m
        bounds, count = dominated_boxes_device(Y, ref)
        out[f"acq/boxes-m{m}/bounds"], out[f"acq/boxes-m{m}/count"] = bounds.cpu(), count.cpu()
        out[f"acq/boxes-m{m}/hypervolume_front"] = hypervolume_front_device(Y, ref).cpu()


if len(sys.argv) > 2 and sys.argv[1] == "--dump":
    sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]
    import torch

    from dkg_amd import DiscreteKnowledgeGradient
    from dkg_amd.synthetic import WORKLOADS, make_problem

    out = {}
    dump_acquisition(out)
    for name in () if "--acq-only" in sys.argv else ("small", "parity6d", "headline", "headline_nd", "stress"):
        w = WORKLOADS[name]
        model, D, X, W = make_problem(w)
        for target in (None, 1):
            acq = DiscreteKnowledgeGradient(model, D, W, target_output_ix=target)
            Xd = X.cuda().unsqueeze(-2)
            out[f"{name}/{target}/kg"] = acq(Xd).cpu()
            out[f"{name}/{target}/pairs"] = acq.forward_pairs(X.cuda()).cpu()
            if name in ("small", "headline"):
                Xg = X[:16].cuda().unsqueeze(-2).requires_grad_(True)
                (g,) = torch.autograd.grad(acq(Xg).sum(), Xg)
                out[f"{name}/{target}/grad"] = g.cpu()
    torch.save(out, sys.argv[2])
    sys.exit(0)

import torch  # noqa: E402

flags = [a for a in sys.argv[3:] if a == "--acq-only"]
res = []
for i, lib in enumerate(sys.argv[1:3]):
    path = f"/tmp/ab_{i}.pt"
    # a build that faults, aborts or runs out of time ends the comparison: check=True raises before the next starts
    subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--dump", path] + flags, check=True,
                   env=dict(os.environ, DKG_LIB=lib))
    res.append(torch.load(path))
bad, table = 0, {}
bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.double else t  # noqa: E731
assert sorted(res[0]) == sorted(res[1])
for k in res[0]:
    a, b = res[0][k], res[1][k]
    # torch.equal on the bit patterns: a NaN equals itself and -0.0 differs from 0.0
    same = a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    bad += not same
    diff = (a.double() - b.double()).abs().nan_to_num(0.0, 0.0, 0.0).max().item() if a.shape == b.shape and a.numel() else 0.0
    table[k] = {"same_bits": bool(same), "max_abs_diff": diff, "shape": list(a.shape)}
    print(f"{k:44s} {'same bits' if same else 'DIFFERENT'}  max|diff| {diff:.3e}")
print("all identical" if bad == 0 else f"{bad} outputs differ")
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump({"libs": sys.argv[1:3], "outputs": len(table), "different": bad, "table": table}, f, indent=1)
sys.exit(1 if bad else 0)
