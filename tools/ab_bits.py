"""Bit-identity of two builds of libdkg.so (DKG_LIB A/B): forward KG, KG per pair and the value+gradient
path on several workloads, then the acquisition layer (posterior mean, sample paths, NSGA-II, ranks, JES, HVKG,
boxes) at small ragged shapes in every dimension bucket and covariance family, then the core entries' host side
(state preparation with a jitter retry inside the batch, the MLL, an append, plans that take every section of
the plan workspace, and under envelope/ the envelope kernels' modes at tiny shapes).

Run on the GPU box from the repo root:
    python tools/ab_bits.py <libA.so> <libB.so> [--acq-only|--core-only] [--json OUT]
Each build runs in its own subprocess under a time limit (the library is loaded once per process), the second
only after the first ended well; prints, per output, whether the two builds agree bit for bit, and with --json
writes the table.  --acq-only skips the KG workloads, --core-only runs the core entries alone.
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


def dump_core(out):
    """What a host-side change of csrc/dkg_abi.hip can move without changing a workspace size: an interior offset of
    the plan, MLL or append workspace, or the sequence of the batched factorisation.  State, MLL and append at
    n = (37, 36, 16), the third output needing the first jitter; the plans at n = (37, 36, 35), B = 17."""
    import torch

    from dkg_amd.fit import DeviceMll
    from dkg_amd.gp_state import DeviceGPState
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    dev, d = torch.device("cuda", 0), 3
    g = torch.Generator().manual_seed(2024)
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.double)  # noqa: E731
    randn = lambda n: torch.randn(n, generator=g, dtype=torch.double)  # noqa: E731
    Xj = rnd(12, d)
    Xj = torch.cat([Xj, Xj[:4]])  # duplicated inputs under a slightly negative shift (tests/test_gpu_state.py)
    first = [SingleTaskGPState(rnd(37, d), randn(37), 0.3 + rnd(d), 2.0, 1e-3, 0.1, "matern", 2.5),
             SingleTaskGPState(rnd(36, d), randn(36), 0.3 + rnd(d), 0.7, 1e-4, -0.3, "rbf")]
    jittered = first + [SingleTaskGPState(Xj, randn(16), 0.5, 1.0, -5e-9, 0.0)]
    plain = first + [SingleTaskGPState(rnd(35, d), randn(35), 0.3 + rnd(d), 1.3, 1e-2, 0.2, "matern", 1.5)]
    D = rnd(50, d)

    def caches(key, outputs):
        for i, c in enumerate(outputs):
            for name in ("L", "Linv", "alpha", "root_frag", "disc_frag", "disc_mean"):
                out[f"{key}/{i}/{name}"] = getattr(c, name).cpu()
            out[f"{key}/{i}/jitter"] = torch.tensor([c.jitter], dtype=torch.double)

    state = DeviceGPState(ModelListGPState(*jittered), D, dev)
    assert state.outputs[2].jitter > 0.0 and state.outputs[0].jitter == 0.0, "the retry did not run inside the batch"
    caches("core/state", state.outputs)
    mll = DeviceMll([s.train_x for s in jittered], [s.train_y for s in jittered], [2.5, float("inf"), 2.5], dev)
    for name, a in zip(("value", "grad", "jitter"), mll.evaluate(
            [s.mean_constant for s in jittered], [s.lengthscale.tolist() for s in jittered],
            [s.outputscale for s in jittered], [s.noise for s in jittered])):
        out["core/mll/" + name] = torch.from_numpy(a)
    assert out["core/mll/jitter"][2] > 0.0
    caches("core/append", [state.with_observation(0, rnd(d), y=0.3).outputs[0]])

    X = rnd(17, d).to(dev)
    W = lambda S: 0.1 + rnd(S, 3)  # noqa: E731
    st = DeviceGPState(ModelListGPState(*plain), D, dev)
    out["core/f32/kg"] = st.plan(W(3), None, 17, f32=True).forward(X).cpu()
    every = [None, 0, 1, 2]
    for part, t in zip(("kg", "pairs", "hull_sizes"), st.plan(W(3), None, 17, targets=every).forward_stats(X)):
        out["core/targets/" + part] = t.cpu()
    for part, t in zip(("kg", "grad"), st.plan(W(3), None, 17, grad=True, targets=every).forward_grad(X)):
        out["core/targets_grad/" + part] = t.cpu()
    for part, t in zip(("kg", "grad"), st.plan(W(3), None, 17, grad=True, grad_rows="global").forward_grad(X)):
        out["core/global_rows/" + part] = t.cpu()
    for S in (9, 17):  # envelope split 2 and 3: wg_part, wg_gpart, tickets
        w = W(S)
        for part, t in zip(("kg", "pairs", "hull_sizes"), st.plan(w, 1, 17).forward_stats(X)):
            out[f"core/S{S}/{part}"] = t.cpu()
        for part, t in zip(("kg", "grad"), st.plan(w, 1, 17, grad=True).forward_grad(X)):
            out[f"core/S{S}/grad_{part}"] = t.cpu()
    # N + 1 > 64 * 33: streaming, no intercept scratch
    wide = DeviceGPState(ModelListGPState(*plain), rnd(2112, d), dev)
    out["core/N2112/kg"] = wide.plan(W(3), None, 3).forward(X[:3]).cpu()
    # 32 batches of 16: the K(x, X) fill by candidate count, with its kx section
    Xb, kg = rnd(512, d).to(dev), torch.empty(512, dtype=torch.double, device=dev)
    DeviceGPState(ModelListGPState(*plain), rnd(20, d), dev).plan(W(3), None, 512).forward_batches_into(Xb, kg, 16)
    out["core/batches/kg"] = kg.cpu()
    dump_envelope(out, g)


def dump_envelope(out, g):
    """The envelope body's modes the cases above do not reach, at tiny shapes: every output bucket but 3, narrow
    and wide workgroups, the list path and the forced walk, a coincident candidate, the slot buckets, the
    streaming kernels (staged or not, the chain off, the gradient) and the fused launch."""
    import torch

    from dkg_amd.gp_state import DeviceGPState
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    dev, d = torch.device("cuda", 0), 3
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.double)  # noqa: E731
    kinds = (("matern", 2.5), ("rbf", 2.5), ("matern", 1.5), ("matern", 0.5), ("rbf", 2.5))

    def models(m, n=20):
        return ModelListGPState(*[
            SingleTaskGPState(rnd(n - i, d), torch.randn(n - i, generator=g, dtype=torch.double), 0.3 + rnd(d),
                              0.7 + 0.3 * i, 1e-2, 0.1 * i, kinds[i][0], kinds[i][1]) for i in range(m)])

    def stats(key, plan, X):
        for part, t in zip(("kg", "pairs", "hull_sizes"), plan.forward_stats(X)):
            out[f"{key}/{part}"] = t.cpu()

    def grads(key, plan, X):
        for part, t in zip(("kg", "grad"), plan.forward_grad(X)):
            out[f"{key}/grad_{part}"] = t.cpu()

    X = rnd(5, d).to(dev)
    for m in (1, 2, 4, 5):
        st = DeviceGPState(models(m), rnd(50, d), dev)
        for S in (3, 9):
            w = 0.1 + rnd(S, m)
            for walk in (False, True):
                key = f"envelope/m{m}-S{S}{'-walk' if walk else ''}"
                stats(key, st.plan(w, None, 5, force_walk=walk), X)
                grads(key, st.plan(w, None, 5, grad=True, force_walk=walk), X)
    # a candidate equal to a discretisation point: line 0 from its record
    D = rnd(50, d)
    st = DeviceGPState(models(2), D, dev)
    Xc = torch.cat([X[:2].cpu(), D[7:8], X[2:4].cpu()]).to(dev)
    stats("envelope/coincident", st.plan(0.1 + rnd(3, 2), None, 5), Xc)
    grads("envelope/coincident", st.plan(0.1 + rnd(3, 2), None, 5, grad=True), Xc)
    fused = st.plan(0.1 + rnd(3, 2), None, 5, fused=True)
    assert fused.fused, "the library declined the fused launch at this shape"
    out["envelope/fused/kg"] = fused.forward(X).cpu()
    for N in (200, 600, 1500):  # slot buckets 8, 17, 33
        sn = DeviceGPState(models(2), rnd(N, d), dev)
        stats(f"envelope/N{N}", sn.plan(0.1 + rnd(3, 2), None, 3), X[:3])
        grads(f"envelope/N{N}", sn.plan(0.1 + rnd(3, 2), None, 3, grad=True), X[:3])
    for m in (1, 5):  # streaming, not staged-streaming
        sn = DeviceGPState(models(m), rnd(2112, d), dev)
        out[f"envelope/N2112-m{m}/kg"] = sn.plan(0.1 + rnd(3, m), None, 3).forward(X[:3]).cpu()
    sn = DeviceGPState(models(3), rnd(2112, d), dev)
    out["envelope/N2112-m3-no_chain/kg"] = sn.plan(0.1 + rnd(3, 3), None, 3, no_chain=True).forward(X[:3]).cpu()
    sn = DeviceGPState(models(2), rnd(2112, d), dev)
    grads("envelope/N2112-m2", sn.plan(0.1 + rnd(3, 2), None, 3, grad=True), X[:3])


if len(sys.argv) > 2 and sys.argv[1] == "--dump":
    sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]
    import torch

    from dkg_amd import DiscreteKnowledgeGradient
    from dkg_amd.synthetic import WORKLOADS, make_problem

    out = {}
    dump_core(out)
    if "--core-only" not in sys.argv:
        dump_acquisition(out)
    only = "--acq-only" in sys.argv or "--core-only" in sys.argv
    for name in () if only else ("small", "parity6d", "headline", "headline_nd", "stress"):
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

flags = [a for a in sys.argv[3:] if a in ("--acq-only", "--core-only")]
res = []
for i, lib in enumerate(sys.argv[1:3]):
    path = f"/tmp/ab_{i}.pt"
    # a build that faults, aborts or runs out of time ends the comparison: check=True raises before the next starts
    subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--dump", path] + flags, check=True,
                   env=dict(os.environ, DKG_LIB=lib))
    res.append(torch.load(path))
bad, table = 0, {}
bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.double and t.dim() else t  # noqa: E731
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
