"""One observation appended to the device GP state without refactorising (dkg_append_observation,
gp_state.append_observation, DeviceGPState.with_observation, set_incremental_state).

Every case starts from a full preparation (prepare_outputs) at n0 and appends the remaining rows of a
fixed data set one at a time.  The factor state is held to the backward-error bounds of test_gpu_state.py,
which do not depend on the conditioning:
  |L' L'^T - K'|_max      <= 64 eps n |K'|_max
  |L' L'^-1 - I|_max      <= 64 eps n |L'|_max |L'^-1|_max
  |K' alpha' - r'|_max    <= 64 eps n (|K'|_max |alpha'|_max + |r'|_max)
and lines, KG and gradient on the appended state to the oracle of the full model at the tolerances the
parity tests state (helpers.LINE_RTOL, stated_tol, grad_tol).
"""

import ctypes
from functools import lru_cache

import pytest
import torch

import dkg_amd
from dkg_amd import DiscreteKnowledgeGradient, _lib, clear_state_cache
from dkg_amd.errors import NotPSDError, UnsupportedError
from dkg_amd.gp_state import DeviceGPState, _pad16, append_observation, prepare_outputs
from dkg_amd.model import ModelListGPState, SingleTaskGPState
from dkg_amd.synthetic import WORKLOADS, make_problem
from helpers import LINE_RTOL, assert_within, grad_scale, grad_tol, line_gap, load_golden, stated_tol, to_oracle
from oracle.gp import OutputGP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = torch.finfo(torch.double).eps


def problem(n, d=2, ls=0.3, s=1.0, noise=1e-4, seed=0, c=0.25):
    """test_gpu_state.py's generator."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.double)
    y = torch.randn(n, generator=g, dtype=torch.double)
    return SingleTaskGPState(X, y, ls, s, noise, c)


def head(st: SingleTaskGPState, n: int) -> SingleTaskGPState:
    return SingleTaskGPState(st.train_x[:n], st.train_y[:n], st.lengthscale, st.outputscale, st.noise,
                             st.mean_constant, st.kernel, st.nu, st.y_mean, st.y_std)


def host_K(st, jit=0.0):
    og = OutputGP(st.train_x, st.train_y, st.lengthscale, st.outputscale, st.noise, st.mean_constant, st.kernel,
                  st.nu)
    K = og.covar(st.train_x, st.train_x)
    return K + (st.noise + jit) * torch.eye(K.shape[0], dtype=torch.double)


def chain(st: SingleTaskGPState, n0: int, D: torch.Tensor):
    """prepare_outputs at n0, then the rows n0 .. n of st appended one at a time."""
    (cache,) = prepare_outputs([head(st, n0)], D)
    for k in range(n0, st.num_train):
        cache = append_observation(cache, D, st.train_x[k], st.train_y[:k + 1])
    torch.cuda.synchronize()
    return cache


def disc_points(N, d=2, seed=21):
    return torch.rand(N, d, generator=torch.Generator().manual_seed(seed), dtype=torch.double).to(DEV)


@lru_cache(maxsize=None)
def chained(n0, n1):
    st = problem(n1, noise=1e-2)
    return st, chain(st, n0, disc_points(50))


def frag_padding(frag: torch.Tensor, rows: int, n: int) -> torch.Tensor:
    """The padding entries (row >= rows or column >= n) of a fragment-packed (rows x n) matrix
    (include/dkg.h "Data layout": F[t][j][l][h] = P[16 t + (l & 15)][4 (2 j + h) + (l >> 4)])."""
    rp, np_ = _pad16(rows), _pad16(n)
    F = frag[: rp * np_].reshape(rp // 16, np_ // 8, 64, 2)
    t = torch.arange(rp // 16).reshape(-1, 1, 1, 1)
    j = torch.arange(np_ // 8).reshape(1, -1, 1, 1)
    l = torch.arange(64).reshape(1, 1, -1, 1)
    h = torch.arange(2).reshape(1, 1, 1, -1)
    row = 16 * t + (l & 15)
    col = 4 * (2 * j + h) + (l >> 4)
    pad = (row >= rows) | (col >= n)
    return F[pad.expand_as(F)]


def check_bound_1(st, L, jit=0.0):
    n = st.num_train
    K = host_K(st, jit)
    assert (L @ L.T - K).abs().max() <= 64 * EPS * n * K.abs().max()
    return K


CHAINS = [(1, 4), (15, 17), (31, 33), (63, 65), (100, 105), (255, 256), (1023, 1024)]


@pytest.mark.parametrize("n0,n1", CHAINS)
def test_factor_state_after_chain(n0, n1):
    """Smallest n, the n_pad crossing, the Cholesky's block width, both, neither, the headline n, the limit."""
    lib = _lib.load()
    st, cache = chained(n0, n1)
    n = n1
    L, linv, alpha = cache.L.cpu(), cache.Linv.cpu(), cache.alpha.cpu()
    assert L.shape == (n, n) and linv.shape == (n, n) and alpha.shape == (_pad16(n),)
    assert cache.state.num_train == n and cache.struct.n == n and cache.jitter == 0.0
    K = check_bound_1(st, L)
    scale = 64 * EPS * n
    assert torch.equal(L.triu(1), torch.zeros_like(L))
    assert (L @ linv - torch.eye(n, dtype=torch.double)).abs().max() <= scale * L.abs().max() * linv.abs().max()
    r = st.train_y - st.mean_constant
    res = (K @ alpha[:n] - r).abs().max()
    assert res <= scale * (K.abs().max() * alpha[:n].abs().max() + r.abs().max())
    assert torch.equal(alpha[n:], torch.zeros(_pad16(n) - n, dtype=torch.double))
    # forward errors against LAPACK (well conditioned: noise 1e-2), as test_prepare_matches_lapack
    L_ref = torch.linalg.cholesky(K)
    torch.testing.assert_close(L, L_ref, rtol=1e-10, atol=1e-11 * L_ref.abs().max().item())
    a_ref = torch.cholesky_solve(r.unsqueeze(-1), L_ref).squeeze(-1)
    torch.testing.assert_close(alpha[:n], a_ref, rtol=1e-8, atol=1e-9 * a_ref.abs().max().item())
    # root_frag is dkg_pack_root of the new L^{-T}, bit for bit
    R = cache.Linv.T.contiguous()
    ref = torch.empty(lib.dkg_frag_elems(n, n), dtype=torch.double, device=DEV)
    _lib.check(lib.dkg_pack_root(_lib.ptr(R), n, _lib.ptr(ref), torch.cuda.current_stream(DEV).cuda_stream),
               "dkg_pack_root")
    torch.cuda.synchronize()
    assert torch.equal(cache.root_frag, ref)
    # N = 50 (not a multiple of 16): the padding of disc_frag and disc_mean is exactly zero
    pad = frag_padding(cache.disc_frag.cpu(), 50, n)
    assert pad.numel() == 64 * _pad16(n) - 50 * n and torch.equal(pad, torch.zeros_like(pad))
    assert torch.equal(cache.disc_mean[50:64].cpu(), torch.zeros(14, dtype=torch.double))
    # the new column and the means against the host's Q_D = K(D, X) L^{-T}, mu_D = c + K(D, X) alpha
    og = OutputGP(st.train_x, st.train_y, st.lengthscale, st.outputscale, st.noise, st.mean_constant)
    KD = og.covar(disc_points(50).cpu(), st.train_x)
    Q = torch.linalg.solve_triangular(L_ref, KD.T, upper=False).T
    F = cache.disc_frag.cpu()[: 64 * _pad16(n)].reshape(4, _pad16(n) // 8, 64, 2)
    dense = F.permute(0, 2, 1, 3)  # [t][l][j][h] -> row 16 t + (l & 15), column 8 j + 4 h + (l >> 4)
    got = torch.empty(64, _pad16(n), dtype=torch.double)
    for l in range(64):
        got[(l & 15)::16, (l >> 4)::4] = dense[:, l].reshape(4, -1)
    torch.testing.assert_close(got[:50, :n], Q, rtol=1e-8, atol=1e-9 * Q.abs().max().item())
    torch.testing.assert_close(cache.disc_mean[:50].cpu(), st.mean_constant + KD @ a_ref, rtol=1e-8,
                               atol=1e-9 * a_ref.abs().max().item())


@pytest.mark.parametrize("n0,n1", [(15, 17), (100, 101)])
def test_append_without_discretisation(n0, n1):
    """N = 0: the factor state alone (no discretisation pass)."""
    st = problem(n1, noise=1e-2)
    cache = chain(st, n0, torch.empty(0, 2, dtype=torch.double, device=DEV))
    check_bound_1(st, cache.L.cpu())
    pad = frag_padding(cache.disc_frag.cpu(), 0, n1)
    assert pad.numel() == 0
    ref = chained(15, 17)[1] if (n0, n1) == (15, 17) else None
    if ref is not None:  # the factor state does not depend on the discretisation
        assert torch.equal(cache.L, ref.L) and torch.equal(cache.alpha, ref.alpha)


@pytest.mark.parametrize("kernel,nu", [("matern", 0.5), ("matern", 1.5), ("rbf", None)])
def test_append_other_kernels(kernel, nu):
    g = torch.Generator().manual_seed(5)
    X = torch.rand(72, 3, generator=g, dtype=torch.double)
    st = SingleTaskGPState(X, torch.randn(72, generator=g, dtype=torch.double), [0.3, 0.5, 0.9], 2.0, 1e-3, -0.4,
                           kernel, 2.5 if nu is None else nu)
    cache = chain(st, 70, disc_points(20, d=3))
    check_bound_1(st, cache.L.cpu())


# --------------------------------------------------------------------------------------------------
# lines, KG and the gradient on an appended state against the oracle of the full model

@lru_cache(maxsize=None)
def appended_workload(name, n0, ncand):
    model, D, X, W = make_problem(WORKLOADS[name])
    X = X if ncand is None else X[:ncand]
    start = ModelListGPState(*[head(m, n0) for m in model.models])
    st = DeviceGPState(start, D, DEV)
    for i, m in enumerate(model.models):
        for k in range(n0, m.num_train):
            st = st.with_observation(i, m.train_x[k], y=m.train_y[k])
    return model, to_oracle(model), D, X, W, st


@lru_cache(maxsize=None)
def oracle_lines(name, n0, ncand, target):
    from oracle.discretekg import kg_pairs_from_lines, lines_batched

    _, om, D, X, W, _ = appended_workload(name, n0, ncand)
    a, b = lines_batched(om, X, D, W, target)
    return a, b, kg_pairs_from_lines(a, b).mean(-1)


@pytest.mark.parametrize("target", [None, 0, 1])
@pytest.mark.parametrize("name,n0,ncand,lines", [("small", 40, None, True), ("parity6d", 100, None, True),
                                                  ("headline", 230, 16, False)])
def test_lines_and_kg_on_appended_state(name, n0, ncand, lines, target):
    """small 40 -> 64 and parity6d 100 -> 128: every candidate, lines within LINE_RTOL and KG within the
    stated tolerance; headline 230 -> 256: the first 16 candidates, KG only (its conditioning leaves two
    fp64 builds of the lines 4e-9 apart, too close to LINE_RTOL to assert)."""
    model, om, D, X, W, st = appended_workload(name, n0, ncand)
    assert [c.state.num_train for c in st.outputs] == [m.num_train for m in model.models]
    a_ref, b_ref, kg_ref = oracle_lines(name, n0, ncand, target)
    plan = st.plan(W, target, X.shape[0])
    Xd = X.to(DEV)
    kg = plan.forward(Xd).cpu()
    a_dev, b_dev = plan.lines(Xd)
    da, db = line_gap(a_dev, b_dev, a_ref, b_ref)
    rel_a = float(da.max() / a_ref.abs().max().clamp_min(1e-300))
    rel_b = float(db.max() / b_ref.abs().max().clamp_min(1e-300))
    tol = stated_tol(kg_ref, a_ref.abs().amax(dim=(-1, -2)))
    print(f"{name} target={target}: line rel gap {rel_a:.3e} / {rel_b:.3e}, KG max err "
          f"{float((kg - kg_ref).abs().max()):.3e}, worst err/tol {float(((kg - kg_ref).abs() / tol).max()):.3g}")
    if lines:
        assert rel_a <= LINE_RTOL and rel_b <= LINE_RTOL, (rel_a, rel_b)
    assert_within(kg, kg_ref, tol, "KG on the appended state")


def test_gradient_on_appended_state():
    from oracle.discretekg import discrete_kg_batched

    _, om, D, X, W, st = appended_workload("small", 40, None)
    X = X[:12]
    Xr = X.clone().requires_grad_(True)
    kg_ref, _ = discrete_kg_batched(om, Xr, D, W, None)
    (g_ref,) = torch.autograd.grad(kg_ref.sum(), Xr)
    _, g = st.plan(W, None, 16, grad=True).forward_grad(X.to(DEV))
    err = (g.cpu() - g_ref).abs()
    tol = grad_tol(g_ref, grad_scale(om, X, D, W, None))
    assert bool((err <= tol).all()), f"max err {err.max():.3e}, worst err/tol {(err / tol).max():.3f}"


# --------------------------------------------------------------------------------------------------

def test_update_is_functional():
    """The other outputs' caches are shared, the old state is untouched: a plan made before the append
    gives the same bits after it."""
    model, D, X, W = make_problem(WORKLOADS["small"])
    old = DeviceGPState(model, D, DEV)
    plan = old.plan(W, None, 32)
    Xd = X.to(DEV)
    before = plan.forward(Xd).clone()
    x = torch.tensor([0.31, 0.62], dtype=torch.double)
    new = old.with_observation(1, x, y=0.5)
    assert new is not old and new.model is not old.model and isinstance(new.model, ModelListGPState)
    assert new.outputs[0] is old.outputs[0]
    for name in ("train_x", "alpha", "root_frag", "disc_frag", "disc_mean", "L", "Linv"):
        assert getattr(new.outputs[0], name).data_ptr() == getattr(old.outputs[0], name).data_ptr(), name
        assert getattr(new.outputs[1], name).data_ptr() != getattr(old.outputs[1], name).data_ptr(), name
    assert old.outputs[1].state.num_train == 64 and new.outputs[1].state.num_train == 65
    assert new.model.models[1].train_x.shape == (65, 2) and float(new.model.models[1].train_y[-1]) == 0.5
    assert old.model.models[1].num_train == 64
    after = plan.forward(Xd)
    assert torch.equal(before, after)
    assert not torch.equal(new.plan(W, None, 32).forward(Xd), before)
    with pytest.raises(ValueError):
        old.with_observation(0, x)
    with pytest.raises(IndexError):
        old.with_observation(2, x, y=0.0)


def test_jitter_is_carried():
    """The duplicated-input problem of test_jitter_retry_follows_psd_safe_cholesky (jitter 1e-8): the
    appended row is factored under the same jitter."""
    X = torch.rand(12, 2, generator=torch.Generator().manual_seed(3), dtype=torch.double)
    X = torch.cat([X, X[:4], torch.tensor([[0.37, 0.81]], dtype=torch.double)])
    y = torch.randn(17, generator=torch.Generator().manual_seed(4), dtype=torch.double)
    st = SingleTaskGPState(X, y, 0.5, 1.0, -5e-9, 0.0)
    cache = chain(st, 16, disc_points(20))
    assert cache.jitter == pytest.approx(1e-8)
    check_bound_1(st, cache.L.cpu(), jit=1e-8)


def raw_append(cache, D, x, train_y):
    """dkg_append_observation itself: (status, L', L'^-1, alpha', root_frag', disc_frag', disc_mean')."""
    lib = _lib.load()
    n, d = cache.train_x.shape
    N, n1 = D.shape[0], n + 1
    X = torch.cat([cache.train_x, x.reshape(1, d).to(DEV)])
    y = train_y.to(DEV)
    out = [torch.full((n1, n1), float("nan"), dtype=torch.double, device=DEV) for _ in range(2)]
    out += [torch.full((k,), float("nan"), dtype=torch.double, device=DEV)
            for k in (_pad16(n1), lib.dkg_frag_elems(n1, n1), max(1, lib.dkg_frag_elems(N, n1)), max(16, _pad16(N)))]
    work = torch.empty(lib.dkg_append_workspace(n, N), dtype=torch.uint8, device=DEV)
    status = lib.dkg_append_observation(cache.struct, d, _lib.ptr(cache.L), _lib.ptr(cache.Linv), _lib.ptr(D), N,
                                        _lib.ptr(X), _lib.ptr(y), cache.jitter, *[_lib.ptr(t) for t in out],
                                        _lib.ptr(work), work.numel(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return (status, *out)


def not_pd_problem():
    X = torch.rand(8, 2, generator=torch.Generator().manual_seed(9), dtype=torch.double)
    y = torch.randn(9, generator=torch.Generator().manual_seed(10), dtype=torch.double)
    return SingleTaskGPState(torch.cat([X, X[:1]]), y, 0.5, 1.0, -1e-9, 0.0)


def test_not_positive_definite():
    """8 distinct points with noise -1e-9 and a copy of point 0 appended: the Schur complement is about
    -2e-9.  The C call says so, with_observation raises, and the incremental shared_state falls back to the
    full build (whose jitter policy repairs it)."""
    st = not_pd_problem()
    D = disc_points(20)
    (cache,) = prepare_outputs([head(st, 8)], D)
    assert cache.jitter == 0.0
    assert raw_append(cache, D, st.train_x[8], st.train_y)[0] == _lib.DKG_ERR_NOT_PD
    dev_state = DeviceGPState(ModelListGPState(head(st, 8)), D, DEV)
    with pytest.raises(NotPSDError, match="not positive definite"):
        dev_state.with_observation(0, st.train_x[8], y=float(st.train_y[8]))
    Xc = torch.rand(6, 1, 2, generator=torch.Generator().manual_seed(12), dtype=torch.double).to(DEV)
    clear_state_cache()
    cold = DiscreteKnowledgeGradient(ModelListGPState(st), D.cpu(), device=DEV)(Xc)
    clear_state_cache()
    dkg_amd.reset_state_stats()
    prev = dkg_amd.set_incremental_state(True)
    try:
        DiscreteKnowledgeGradient(ModelListGPState(head(st, 8)), D.cpu(), device=DEV)(Xc)
        got = DiscreteKnowledgeGradient(ModelListGPState(st), D.cpu(), device=DEV)(Xc)
    finally:
        dkg_amd.set_incremental_state(prev)
        clear_state_cache()
    stats = dkg_amd.state_stats()
    assert stats["append_fallbacks"] == 1 and stats["appends"] == 0 and stats["full_builds"] == 2
    assert torch.equal(got, cold)


def test_limit():
    """n = 1024 is the most the preparation supports: appending to it raises UnsupportedError."""
    st, cache = chained(1023, 1024)
    with pytest.raises(UnsupportedError, match="1024"):
        append_observation(cache, disc_points(50), torch.tensor([0.5, 0.5]), torch.zeros(1025))
    assert raw_append(cache, disc_points(50), torch.tensor([0.5, 0.5], dtype=torch.double),
                      torch.zeros(1025, dtype=torch.double))[0] == _lib.DKG_ERR_UNSUPPORTED


@pytest.mark.parametrize("n", [64, 100])
def test_append_is_deterministic(n):
    """The same append twice: equal bits in every output array (n = 64 crosses n_pad)."""
    st = problem(n + 1, noise=1e-2)
    D = disc_points(50)
    (cache,) = prepare_outputs([head(st, n)], D)
    a = raw_append(cache, D, st.train_x[n], st.train_y)
    b = raw_append(cache, D, st.train_x[n], st.train_y)
    assert a[0] == _lib.DKG_OK and b[0] == _lib.DKG_OK
    for u, v in zip(a[1:], b[1:]):
        assert not bool(torch.isnan(u).any()) and torch.equal(u, v)


def test_incremental_switch():
    """Off (the default): a grown model is a full build with the bits of a fresh DeviceGPState.  On: the rows
    are appended and the KG is within the stated tolerance of the cold build."""
    model, D, X, W = make_problem(WORKLOADS["small"])
    Xd = X.to(DEV)
    base = ModelListGPState(head(model.models[0], 63), model.models[1])
    both = ModelListGPState(head(model.models[0], 63), head(model.models[1], 62))
    cold_plan = DeviceGPState(model, D, DEV).plan(W, None, 32)
    cold = cold_plan.forward(Xd)
    amax = cold_plan.lines(Xd)[0].abs().amax(dim=(-1, -2)).cpu()
    assert dkg_amd.gp_state.incremental_state() is False
    clear_state_cache()
    dkg_amd.reset_state_stats()
    try:
        DiscreteKnowledgeGradient(base, D, W, device=DEV)(Xd.unsqueeze(-2))
        off = DiscreteKnowledgeGradient(model, D, W, device=DEV)(Xd.unsqueeze(-2))
        assert dkg_amd.state_stats() == {"full_builds": 2, "appends": 0, "append_fallbacks": 0}
        assert torch.equal(off, cold)
        clear_state_cache()
        dkg_amd.reset_state_stats()
        assert dkg_amd.set_incremental_state(True) is False
        DiscreteKnowledgeGradient(base, D, W, device=DEV)(Xd.unsqueeze(-2))
        on = DiscreteKnowledgeGradient(model, D, W, device=DEV)(Xd.unsqueeze(-2))
        assert dkg_amd.state_stats() == {"full_builds": 1, "appends": 1, "append_fallbacks": 0}
        assert_within(on, cold.cpu(), stated_tol(cold.cpu(), amax), "KG, appended against cold")
        # the same model again: an exact fingerprint match, nothing is built
        acq = DiscreteKnowledgeGradient(model, D, W, device=DEV)
        assert dkg_amd.state_stats()["appends"] == 1 and torch.equal(acq(Xd.unsqueeze(-2)), on)
        # every output grown (a full evaluation, here by 1 and by 2 rows): one append per added row
        clear_state_cache()
        dkg_amd.reset_state_stats()
        DiscreteKnowledgeGradient(both, D, W, device=DEV)(Xd.unsqueeze(-2))
        full = DiscreteKnowledgeGradient(model, D, W, device=DEV)(Xd.unsqueeze(-2))
        assert dkg_amd.state_stats() == {"full_builds": 1, "appends": 3, "append_fallbacks": 0}
        assert_within(full, cold.cpu(), stated_tol(cold.cpu(), amax), "KG, appended against cold")
        grown = ModelListGPState(*[head(m, 63) for m in model.models])
        clear_state_cache()
        dkg_amd.reset_state_stats()
        DiscreteKnowledgeGradient(grown, D, W, device=DEV)(Xd.unsqueeze(-2))
        DiscreteKnowledgeGradient(model, D, W, device=DEV)(Xd.unsqueeze(-2))
        assert dkg_amd.state_stats()["appends"] == model.num_outputs
    finally:
        dkg_amd.set_incremental_state(False)
        clear_state_cache()


def test_bo_loop_incremental(monkeypatch):
    """The SMOKE loop with the incremental state against the same loop with full rebuilds, on the
    lengthscales0 fixture with noise 1e-4 (the SMOKE default 1e-8 puts the conditioning at ~1e10, where
    DESIGN 8b documents rounding-level drift of later steps)."""
    import dkg_amd.bo_smoke as bo

    state, *_ = load_golden("lengthscales0")
    hyper = dict(length_scales=[0.2, 1.8], output_scales=[1, 50], means=[0, 0], noises=[1e-4, 1e-4])
    per_mode = []
    orig = bo.run_mobo

    def counted(*args, **kwargs):
        dkg_amd.reset_state_stats()
        out = orig(*args, **kwargs)
        per_mode.append(dkg_amd.state_stats())
        return out

    clear_state_cache()
    plain = bo.run_smoke(bo.GPProblem(state, device=DEV), hyper, seed=0, incremental=False)
    clear_state_cache()
    monkeypatch.setattr(bo, "run_mobo", counted)
    inc = bo.run_smoke(bo.GPProblem(state, device=DEV), hyper, seed=0, incremental=True)
    clear_state_cache()
    assert dkg_amd.gp_state.incremental_state() is False  # restored
    assert len(per_mode) == 2 and all(s["appends"] >= 1 for s in per_mode), per_mode
    for mode in ("separate", "full"):
        g, w = inc[mode], plain[mode]
        assert g["obj_index"] == w["obj_index"], mode
        assert g["x"][0] == w["x"][0] and g["acq"][0] == w["acq"][0], mode
        for k in range(1, len(w["x"])):
            assert g["x"][k] == pytest.approx(w["x"][k], abs=2e-3), (mode, k, g["x"][k], w["x"][k])
            assert g["acq"][k] == pytest.approx(w["acq"][k], rel=1e-4, abs=1e-8), (mode, k)
