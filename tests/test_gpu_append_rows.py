"""A block of observations appended to fitted states in one batched update (dkg_append_rows,
gp_state.append_observations, DeviceGPState.with_observations).

Every case starts from a full preparation (prepare_outputs) at n0 and appends the remaining K rows of a fixed
data set in one call.  The factor state is held to the backward-error bounds of test_gpu_state.py /
test_gpu_append.py, which do not depend on the conditioning:
  |L' L'^T - K'|_max      <= 64 eps n |K'|_max
  |L' L'^-1 - I|_max      <= 64 eps n |L'|_max |L'^-1|_max
  |K' alpha' - r'|_max    <= 64 eps n (|K'|_max |alpha'|_max + |r'|_max)
to LAPACK at noise 1e-2 at test_factor_state_after_chain's tolerances, and lines, KG and gradient on the grown
state to the oracle of the full model at the tolerances the parity tests state.
"""

import ctypes
from functools import lru_cache

import pytest
import torch

from append_rows_ref import block_update, covar, dense_from_frag
from dkg_amd import _lib
from dkg_amd.errors import NotPSDError, UnsupportedError
from dkg_amd.gp_state import DeviceGPState, _pad16, append_observations, prepare_outputs
from dkg_amd.model import ModelListGPState, SingleTaskGPState
from dkg_amd.synthetic import WORKLOADS, make_problem
from helpers import LINE_RTOL, assert_within, grad_scale, grad_tol, line_gap, stated_tol, to_oracle
from test_gpu_append import DEV, EPS, check_bound_1, disc_points, frag_padding, head, problem

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (14, 3), (15, 17), (16, 16), (31, 2), (63, 2), (100, 10), (250, 32), (992, 32)]
FAMILY = {"M12": ("matern", 0.5), "M32": ("matern", 1.5), "M52": ("matern", 2.5), "RBF": ("rbf", 2.5)}


def with_family(st, fam):
    kernel, nu = FAMILY[fam]
    return SingleTaskGPState(st.train_x, st.train_y, st.lengthscale, st.outputscale, st.noise, st.mean_constant,
                             kernel, nu)


def grow(st, n0, D):
    """prepare_outputs at n0, then the remaining rows of st in one block update."""
    (old,) = prepare_outputs([head(st, n0)], D)
    (new,) = append_observations([old], D, [st.train_x[n0:]], [st.train_y])
    torch.cuda.synchronize()
    return old, new


@lru_cache(maxsize=None)
def grown_case(n0, K, N=50, d=2, fam="M52"):
    st = with_family(problem(n0 + K, d=d, ls=0.3 * (d / 2) ** 0.5, noise=1e-2), fam)
    D = disc_points(N, d=d)
    return (st, D) + grow(st, n0, D)


def check_state(st, new, D, old=None):
    """Everything the issue asks of one new state."""
    lib = _lib.load()
    n, N = st.num_train, D.shape[0]
    L, linv, alpha = new.L.cpu(), new.Linv.cpu(), new.alpha.cpu()
    assert L.shape == (n, n) and linv.shape == (n, n) and alpha.shape == (_pad16(n),)
    assert new.state.num_train == n and new.struct.n == n and new.jitter == 0.0
    assert torch.equal(new.state.train_x, st.train_x) and torch.equal(new.state.train_y, st.train_y)
    assert torch.equal(new.train_x.cpu(), st.train_x)
    K = check_bound_1(st, L)
    scale = 64 * EPS * n
    assert torch.equal(L.triu(1), torch.zeros_like(L)) and torch.equal(linv.triu(1), torch.zeros_like(L))
    assert (L @ linv - torch.eye(n, dtype=torch.double)).abs().max() <= scale * L.abs().max() * linv.abs().max()
    r = st.train_y - st.mean_constant
    res = (K @ alpha[:n] - r).abs().max()
    assert res <= scale * (K.abs().max() * alpha[:n].abs().max() + r.abs().max())
    assert torch.equal(alpha[n:], torch.zeros(_pad16(n) - n, dtype=torch.double))
    # forward errors against LAPACK (well conditioned: noise 1e-2), as test_factor_state_after_chain
    L_ref = torch.linalg.cholesky(K)
    torch.testing.assert_close(L, L_ref, rtol=1e-10, atol=1e-11 * L_ref.abs().max().item())
    a_ref = torch.cholesky_solve(r.unsqueeze(-1), L_ref).squeeze(-1)
    torch.testing.assert_close(alpha[:n], a_ref, rtol=1e-8, atol=1e-9 * a_ref.abs().max().item())
    # root_frag is dkg_pack_root of the new L^{-T}, bit for bit
    R = new.Linv.T.contiguous()
    ref = torch.empty(lib.dkg_frag_elems(n, n), dtype=torch.double, device=DEV)
    _lib.check(lib.dkg_pack_root(_lib.ptr(R), n, _lib.ptr(ref), torch.cuda.current_stream(DEV).cuda_stream),
               "dkg_pack_root")
    torch.cuda.synchronize()
    assert torch.equal(new.root_frag, ref)
    pad = frag_padding(new.root_frag.cpu(), n, n)
    assert torch.equal(pad, torch.zeros_like(pad))
    if N == 0:
        return
    # the padding of disc_frag and disc_mean is exactly zero
    pad = frag_padding(new.disc_frag.cpu(), N, n)
    assert pad.numel() == _pad16(N) * _pad16(n) - N * n and torch.equal(pad, torch.zeros_like(pad))
    assert torch.equal(new.disc_mean[N:_pad16(N)].cpu(), torch.zeros(_pad16(N) - N, dtype=torch.double))
    # the new columns and the means against the host's Q_D = K(D, X) L^{-T}, mu_D = c + K(D, X) alpha
    KD = covar(st, D.cpu(), st.train_x)
    Q = torch.linalg.solve_triangular(L_ref, KD.T, upper=False).T
    got = dense_from_frag(new.disc_frag.cpu(), N, n)
    torch.testing.assert_close(got[:N, :n], Q, rtol=1e-8, atol=1e-9 * Q.abs().max().item())
    torch.testing.assert_close(new.disc_mean[:N].cpu(), st.mean_constant + KD @ a_ref, rtol=1e-8,
                               atol=1e-9 * a_ref.abs().max().item())
    if old is not None:  # and against the restatement of the update from the old device state
        n0 = old.state.num_train
        QD0 = dense_from_frag(old.disc_frag.cpu(), N, n0)[:N, :n0]
        want = block_update(old.state, old.L.cpu(), old.Linv.cpu(), st.train_x[n0:], st.train_y, D=D.cpu(), QD=QD0)
        torch.testing.assert_close(got[:N, :n], want["QD"], rtol=1e-8, atol=1e-9 * Q.abs().max().item())
        assert torch.equal(got[:N, :n0], QD0)  # the old columns are copied
        torch.testing.assert_close(new.disc_mean[:N].cpu(), want["muD"], rtol=1e-8,
                                   atol=1e-9 * a_ref.abs().max().item())


@pytest.mark.parametrize("n0,K", SHAPES)
def test_factor_state_after_block(n0, K):
    st, D, old, new = grown_case(n0, K)
    check_state(st, new, D, old)


@pytest.mark.parametrize("n0,K,N,d,fam", [(15, 17, 0, 1, "M12"), (14, 3, 16, 6, "M32"), (100, 10, 17, 16, "RBF"),
                                          (31, 2, 50, 6, "M12"), (63, 2, 17, 1, "RBF"), (16, 16, 16, 2, "M32")])
def test_other_sizes_and_families(n0, K, N, d, fam):
    st, D, old, new = grown_case(n0, K, N, d, fam)
    check_state(st, new, D, old)


def test_against_full_preparation():
    """Q_D' and mu_D' of the grown output against prepare_outputs of the grown model (the tolerances of
    test_factor_state_after_chain's host comparison)."""
    for n0, K, N in ((100, 10, 50), (15, 17, 17)):
        st, D, old, new = grown_case(n0, K, N)
        (full,) = prepare_outputs([st], D)
        n = st.num_train
        a, b = dense_from_frag(new.disc_frag.cpu(), N, n), dense_from_frag(full.disc_frag.cpu(), N, n)
        torch.testing.assert_close(a, b, rtol=1e-8, atol=1e-9 * b.abs().max().item())
        torch.testing.assert_close(new.disc_mean.cpu(), full.disc_mean.cpu(), rtol=1e-8,
                                   atol=1e-9 * full.alpha.abs().max().item())
        torch.testing.assert_close(new.L, full.L, rtol=1e-10, atol=1e-11 * full.L.abs().max().item())


# --------------------------------------------------------------------------------------------------
# lines, KG and the gradient on a with_observations state against the oracle of the full model

@lru_cache(maxsize=None)
def grown_workload(which):
    """small (n = 64, m = 2) from 54 rows: output 0 grown by 10 rows ("one"), or every output ("all")."""
    model, D, X, W = make_problem(WORKLOADS["small"])
    grow_ix = [0] if which == "one" else list(range(model.num_outputs))
    start = ModelListGPState(*[head(m, 54) if i in grow_ix else m for i, m in enumerate(model.models)])
    st = DeviceGPState(start, D, DEV)
    for i in grow_ix:
        m = model.models[i]
        st = st.with_observations(i, m.train_x[54:], y=m.train_y[54:])
    return model, to_oracle(model), D, X, W, st


@pytest.mark.parametrize("target", [None, 0, 1])
@pytest.mark.parametrize("which", ["one", "all"])
def test_lines_and_kg_on_grown_state(which, target):
    from oracle.discretekg import kg_pairs_from_lines, lines_batched

    model, om, D, X, W, st = grown_workload(which)
    assert [c.state.num_train for c in st.outputs] == [m.num_train for m in model.models]
    a_ref, b_ref = lines_batched(om, X, D, W, target)
    kg_ref = kg_pairs_from_lines(a_ref, b_ref).mean(-1)
    plan = st.plan(W, target, X.shape[0])
    Xd = X.to(DEV)
    kg = plan.forward(Xd).cpu()
    a_dev, b_dev = plan.lines(Xd)
    da, db = line_gap(a_dev, b_dev, a_ref, b_ref)
    rel_a = float(da.max() / a_ref.abs().max().clamp_min(1e-300))
    rel_b = float(db.max() / b_ref.abs().max().clamp_min(1e-300))
    print(f"{which} target={target}: line rel gap {rel_a:.3e} / {rel_b:.3e}")
    assert rel_a <= LINE_RTOL and rel_b <= LINE_RTOL, (rel_a, rel_b)
    assert_within(kg, kg_ref, stated_tol(kg_ref, a_ref.abs().amax(dim=(-1, -2))), "KG on the grown state")


@pytest.mark.parametrize("which", ["one", "all"])
def test_gradient_on_grown_state(which):
    from oracle.discretekg import discrete_kg_batched

    _, om, D, X, W, st = grown_workload(which)
    X = X[:12]
    Xr = X.clone().requires_grad_(True)
    kg_ref, _ = discrete_kg_batched(om, Xr, D, W, None)
    (g_ref,) = torch.autograd.grad(kg_ref.sum(), Xr)
    _, g = st.plan(W, None, 16, grad=True).forward_grad(X.to(DEV))
    err = (g.cpu() - g_ref).abs()
    tol = grad_tol(g_ref, grad_scale(om, X, D, W, None))
    assert bool((err <= tol).all()), f"max err {err.max():.3e}, worst err/tol {(err / tol).max():.3f}"


def test_with_observations_is_functional():
    model, D, X, W = make_problem(WORKLOADS["small"])
    old = DeviceGPState(model, D, DEV)
    Xn = torch.tensor([[0.31, 0.62], [0.7, 0.2], [0.05, 0.9]], dtype=torch.double)
    new = old.with_observations(1, Xn, y=[0.5, -0.25, 1.0])
    assert new is not old and new.outputs[0] is old.outputs[0] and new.outputs[1] is not old.outputs[1]
    assert old.outputs[1].state.num_train == 64 and new.outputs[1].state.num_train == 67
    assert new.model.models[1].train_y[-3:].tolist() == [0.5, -0.25, 1.0]
    same = old.with_observations(1, Xn, train_y=torch.cat([model.models[1].train_y,
                                                           torch.tensor([0.5, -0.25, 1.0], dtype=torch.double)]))
    assert torch.equal(same.outputs[1].alpha, new.outputs[1].alpha)
    with pytest.raises(ValueError):
        old.with_observations(0, Xn)
    with pytest.raises(IndexError):
        old.with_observations(2, Xn, y=[0.0, 0.0, 0.0])


# --------------------------------------------------------------------------------------------------
# the C call itself: several jobs of different shapes in one call

NAMES = ("L", "Linv", "alpha", "root_frag", "disc_frag", "disc_mean")


def raw_rows(items):
    """dkg_append_rows over items of (old cache, D, X2, train_y): (status, info, per job the six output arrays,
    filled with NaN before the call)."""
    lib = _lib.load()
    J = len(items)
    d = items[0][0].train_x.shape[1]
    jobs = (_lib.DkgAppendJob * J)()
    outs, keep = [], []
    for b, (c, D, X2, y) in zip(jobs, items):
        n, K, N = c.train_x.shape[0], X2.shape[0], D.shape[0]
        n1 = n + K
        X = torch.cat([c.train_x, X2.to(DEV)])
        yd = y.to(DEV)
        sizes = ((n1, n1), (n1, n1), (_pad16(n1),), (lib.dkg_frag_elems(n1, n1),),
                 (max(1, lib.dkg_frag_elems(N, n1)),), (max(16, _pad16(N)),))
        out = [torch.full(s, float("nan"), dtype=torch.double, device=DEV) for s in sizes]
        keep.append((X, yd))
        outs.append(out)
        b.o = ctypes.pointer(c.struct)
        b.L, b.Linv, b.disc, b.N, b.K = _lib.ptr(c.L), _lib.ptr(c.Linv), _lib.ptr(D) if N else None, N, K
        b.train_x, b.train_y, b.jitter = _lib.ptr(X), _lib.ptr(yd), float(c.jitter)
        (b.L_new, b.Linv_new, b.alpha_new, b.root_frag_new, b.disc_frag_new,
         b.disc_mean_new) = [_lib.ptr(t) for t in out]
    work = torch.empty(lib.dkg_append_rows_workspace(jobs, J, d), dtype=torch.uint8, device=DEV)
    info = (ctypes.c_int32 * J)()
    status = lib.dkg_append_rows(jobs, J, d, info, _lib.ptr(work), work.numel(),
                                 torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return status, list(info), outs


@lru_cache(maxsize=None)
def batch_items():
    """Five jobs of different n, K, family and N (d = 2)."""
    items, states = [], []
    for n0, K, fam, N, seed in ((14, 3, "M52", 17, 0), (100, 10, "RBF", 50, 1), (15, 17, "M12", 0, 2),
                                (63, 2, "M32", 16, 3), (130, 32, "M52", 50, 4)):
        st = with_family(problem(n0 + K, noise=1e-2, seed=seed), fam)
        D = disc_points(N, seed=30 + seed) if N else torch.empty(0, 2, dtype=torch.double, device=DEV)
        (old,) = prepare_outputs([head(st, n0)], D)
        items.append((old, D, st.train_x[n0:], st.train_y))
        states.append(st)
    return items, states


def as_cache(st, out):
    """The six arrays of raw_rows as check_state reads them."""
    class C:
        pass
    c = C()
    c.L, c.Linv, c.alpha, c.root_frag, c.disc_frag, c.disc_mean = out
    c.state, c.jitter, c.train_x = st, 0.0, st.train_x
    c.struct = type("S", (), {"n": st.num_train})()
    return c


def test_batch_of_different_jobs():
    items, states = batch_items()
    before = [[getattr(c, k).clone() for k in NAMES + ("train_x",)] for c, *_ in items]
    status, info, outs = raw_rows(items)
    assert status == _lib.DKG_OK and info == [0] * 5
    for (c, D, _, _), st, out in zip(items, states, outs):
        for t in out[:4 if D.shape[0] == 0 else 6]:  # N = 0: the discretisation arrays are never written
            assert not bool(torch.isnan(t).any())
        check_state(st, as_cache(st, out), D, c)
    # the same bits alone, in another position, and in a second call
    status2, _, again = raw_rows(items)
    order = [3, 0, 4, 2, 1]
    status3, _, moved = raw_rows([items[k] for k in order])
    assert status2 == _lib.DKG_OK and status3 == _lib.DKG_OK
    for j in range(5):
        _, _, (alone,) = raw_rows([items[j]])
        for k, name in enumerate(NAMES):
            if name.startswith("disc") and items[j][1].shape[0] == 0:
                continue  # N = 0: never written
            assert torch.equal(outs[j][k], alone[k]), (j, name, "alone")
            assert torch.equal(outs[j][k], again[j][k]), (j, name, "second call")
            assert torch.equal(outs[j][k], moved[order.index(j)][k]), (j, name, "moved")
    # out of place: nothing of the old states was written
    for (c, *_), saved in zip(items, before):
        for k, t in zip(NAMES + ("train_x",), saved):
            assert torch.equal(getattr(c, k), t), k


def not_pd_item():
    """test_gpu_append.py's not-PD problem, as a block: 8 distinct points with noise -1e-9, then a fresh point
    and a copy of point 0.  The second pivot of S is about -2e-9: column n + 1 fails, info = n + 2 = 10."""
    X = torch.rand(8, 2, generator=torch.Generator().manual_seed(9), dtype=torch.double)
    y = torch.randn(10, generator=torch.Generator().manual_seed(10), dtype=torch.double)
    fresh = torch.tensor([[0.123, 0.456]], dtype=torch.double)
    st = SingleTaskGPState(torch.cat([X, fresh, X[:1]]), y, 0.5, 1.0, -1e-9, 0.0)
    D = disc_points(20)
    (old,) = prepare_outputs([head(st, 8)], D)
    assert old.jitter == 0.0
    return (old, D, st.train_x[8:], st.train_y)


def test_a_job_that_is_not_positive_definite():
    items, states = batch_items()
    bad = not_pd_item()
    trio = [items[0], bad, items[1]]
    status, info, outs = raw_rows(trio)
    assert status == _lib.DKG_ERR_NOT_PD and info == [0, 10, 0]
    assert b"not positive definite" in _lib.load().dkg_last_error()
    for j, k in ((0, 0), (2, 1)):
        check_state(states[k], as_cache(states[k], outs[j]), items[k][1], items[k][0])
        _, _, (alone,) = raw_rows([items[k]])
        for a, b, name in zip(outs[j], alone, NAMES):
            assert torch.equal(a, b), name
    D = bad[1]
    caches = [bad[0], bad[0]]
    (good_st,) = [SingleTaskGPState(torch.cat([bad[0].state.train_x, bad[2][:1]]), bad[3][:9], 0.5, 1.0, -1e-9, 0.0)]
    with pytest.raises(NotPSDError, match=r"not positive definite.*jobs \[1\]") as e:
        append_observations(caches, D, [bad[2][:1], bad[2]], [bad[3][:9], bad[3]])
    assert e.value.jobs == [1] and e.value.caches[1] is None
    check_bound_1(good_st, e.value.caches[0].L.cpu())
    got = append_observations(caches, D, [bad[2][:1], bad[2]], [bad[3][:9], bad[3]], check=False)
    assert got[1] is None and torch.equal(got[0].L, e.value.caches[0].L)


def test_limits():
    st = problem(1000, noise=1e-2)
    D = disc_points(16)
    (old,) = prepare_outputs([st], D)
    g = torch.Generator().manual_seed(1)
    with pytest.raises(UnsupportedError, match="1024"):
        append_observations([old], D, [torch.rand(32, 2, generator=g, dtype=torch.double)], [torch.zeros(1032)])
    _, _, small, _ = grown_case(14, 3)
    with pytest.raises(UnsupportedError, match="K=33"):
        append_observations([small], D, [torch.rand(33, 2, generator=g, dtype=torch.double)], [torch.zeros(47)])
    with pytest.raises(ValueError):
        append_observations([small], D, [torch.rand(3, 2, generator=g, dtype=torch.double)], [torch.zeros(16)])
