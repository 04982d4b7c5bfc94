"""The wide Pareto-rank path on the GPU (csrc/dkg_pareto.hip: pareto_clear / dom / peel / crowd / order kernels):
rank, crowding and order equal the numpy restatement (tests/pareto_ref.py) and the one-workgroup kernel exactly,
at the smallest shapes at which each kernel can go wrong, beyond the old 2048-point limit, at the 16384-point cap,
inside dkg_pareto_nsga2, and from Python (nondominated_rank, posterior_front_on_points).

Kernel limits the shapes are chosen against: pareto_dom_kernel tiles 256 points x 128 rows; pareto_peel_kernel is
one workgroup of min(1024, Q rounded up to 64) threads with ceil(Q / 1024) points per thread, F in LDS when
8 Q + 16 + 8 Q m bytes <= 160 KiB (8 Q: its two int lists), else read from global memory; the crowding and order
kernels take one wave per point, four per workgroup."""

import contextlib
import functools

import numpy as np
import pytest
import torch

import pareto_ref
import pareto_wide_ref
from dkg_amd import _lib, nondominated_rank, posterior_front_on_points, posterior_mean
from dkg_amd.pareto import PreparedModel, pareto_nsga2, pareto_variation
from helpers import ALL_FAMILIES, grad_case, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXQ = 16384


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


@contextlib.contextmanager
def wide(mode):
    """dkg_debug_pareto_wide(mode) for the block: 1 always wide, 0 never below 2049 points, -1 the rule."""
    lib = _lib.load()
    prev = lib.dkg_debug_pareto_wide(mode)
    assert prev in (-1, 0, 1)
    try:
        yield
    finally:
        lib.dkg_debug_pareto_wide(prev)


def device_rank(Fd, keep, work="own"):
    """dkg_pareto_rank on the device tensor Fd [Q, m]; work: "own" a fresh workspace of the asked size, None no
    workspace, or a uint8 device tensor to use as it is.  -> numpy (rank, crowd, order)."""
    lib = _lib.load()
    Q, m = Fd.shape
    if isinstance(work, str):
        work = torch.empty(int(lib.dkg_pareto_rank_workspace(Q, m)), dtype=torch.uint8, device=DEV)
    rank = torch.full((Q,), -7, dtype=torch.int32, device=DEV)
    crowd = torch.full((Q,), -7.0, dtype=torch.double, device=DEV)
    order = torch.full((Q,), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.dkg_pareto_rank(_lib.ptr(Fd), Q, m, keep, _lib.ptr(rank), _lib.ptr(crowd), _lib.ptr(order),
                                       _lib.ptr(work) or None, 0 if work is None else work.numel(),
                                       torch.cuda.current_stream(DEV).cuda_stream), "dkg_pareto_rank")
    return rank.cpu().numpy(), crowd.cpu().numpy(), order.cpu().numpy()


def rank_input(kind, Q, m):
    """The input kinds of test_gpu_pareto.py."""
    g = np.random.default_rng(1000 * Q + m)
    if kind == "gauss":
        return g.standard_normal((Q, m))
    if kind == "equal":
        return np.full((Q, m), 1.25)
    if kind == "chain":
        return np.repeat(np.arange(Q, dtype=np.float64)[:, None], m, 1)
    if kind == "grid":
        return g.integers(0, 5, size=(Q, m)).astype(np.float64)
    if kind == "dup":
        half = g.standard_normal(((Q + 1) // 2, m))
        return np.concatenate([half, half])[:Q]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def full_reference(kind, Q, m):
    """The restatement with keep = Q, computed once per input; never modified (cut_to_keep copies)."""
    return pareto_ref.rank_crowd_order(rank_input(kind, Q, m), Q)


def keeps(Q):
    return sorted({Q, max(Q // 2, 1), 1})


def assert_same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32
    assert got[0].tolist() == want[0].tolist(), what
    assert got[1].tobytes() == np.ascontiguousarray(want[1]).tobytes(), what
    assert got[2].tolist() == want[2].tolist(), what


# ---------------------------------------------------------------- forced wide at small shapes

def check_forced_wide(kind, Q, m):
    """Mode 1 against the restatement (by its own keep, not the cut) and against mode 0, bit for bit."""
    F = rank_input(kind, Q, m)
    Fd = torch.from_numpy(F).to(DEV)
    for keep in keeps(Q):
        with wide(1):
            got = device_rank(Fd, keep)
        with wide(0):
            narrow = device_rank(Fd, keep)
        assert_same(got, pareto_ref.rank_crowd_order(F, keep), (kind, Q, m, keep))
        assert_same(got, narrow, (kind, Q, m, keep, "mode 0"))
        for a, b in zip(got, narrow):
            assert torch.equal(torch.from_numpy(a), torch.from_numpy(b)) and a.tobytes() == b.tobytes()
        assert int((got[0] >= 0).sum()) >= keep


@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("Q", [1, 2, 63, 64, 65, 257])
def test_forced_wide_gaussian(Q, m):
    """One point, one wave, a wave boundary +-1, a second 256-point tile with one point in it and a partial third
    128-row slice (257), every objective bucket (2, 4, 8) and its clamped tail (m = 1, 3)."""
    check_forced_wide("gauss", Q, m)


@pytest.mark.parametrize("kind,Q,m", [("equal", 65, 3), ("chain", 257, 1), ("chain", 257, 2), ("grid", 257, 2),
                                      ("grid", 64, 8), ("dup", 130, 2), ("dup", 63, 1)])
def test_forced_wide_structured_inputs(kind, Q, m):
    """A peel of one round (equal) and of Q rounds (chain), ties in single objectives (grid), duplicated rows."""
    check_forced_wide(kind, Q, m)


# ---------------------------------------------------------------- beyond the old limit

# (kind, Q, m): the peel's branch.  1024 threads each; 8 Q bytes of lists beside F.
BEYOND = [("gauss", 2049, 2),  # 3 points per thread, F in LDS (16 KiB + 32 KiB)
          ("gauss", 4097, 3),  # 5 points per thread, F in LDS (32 KiB + 96 KiB)
          ("dup", 4097, 3),    # the same branch, duplicated rows
          ("equal", 2049, 2),  # one round, every point a member: the member list full
          ("chain", 2049, 1),  # 2049 rounds of one member, the clamped m = 1 tail
          ("grid", 4097, 8)]   # 5 points per thread, F read from global memory (32 KiB + 256 KiB > 160 KiB)


@pytest.mark.parametrize("kind,Q,m", BEYOND)
def test_beyond_the_one_workgroup_limit(kind, Q, m):
    Fd = torch.from_numpy(rank_input(kind, Q, m)).to(DEV)
    full = full_reference(kind, Q, m)
    for keep in keeps(Q):
        assert_same(device_rank(Fd, keep), pareto_wide_ref.cut_to_keep(*full, keep), (kind, Q, m, keep))


@pytest.mark.parametrize("keep", [MAXQ, 1])
def test_the_cap_on_a_tiled_input(keep):
    """Q = 16384, m = 2: 16 points per thread in the peel, F (256 KiB) read from global memory, 64 x 128
    workgroups of dominator counts.  The expectation is the closed form of tests/pareto_wide_ref.py."""
    base = pareto_wide_ref.tiled_base()
    F = pareto_wide_ref.tiled_input(base, MAXQ // 64)
    assert F.shape == (MAXQ, 2)
    got = device_rank(torch.from_numpy(F).to(DEV), keep)
    assert_same(got, pareto_wide_ref.tiled_expected(base, MAXQ // 64, keep), keep)


def test_two_calls_on_one_workspace():
    """The clear runs on every call: a smaller, different problem on a used workspace gives its own result."""
    lib = _lib.load()
    work = torch.empty(int(lib.dkg_pareto_rank_workspace(4097, 3)), dtype=torch.uint8, device=DEV)
    big = torch.from_numpy(rank_input("gauss", 4097, 3)).to(DEV)
    small_np = rank_input("grid", 300, 2)
    small = torch.from_numpy(small_np).to(DEV)
    with wide(1):
        first = device_rank(big, 4097, work)
        second = device_rank(small, 150, work)
        third = device_rank(big, 1, work)
    full = full_reference("gauss", 4097, 3)
    assert_same(first, full, "first")
    assert_same(second, pareto_ref.rank_crowd_order(small_np, 150), "second")
    assert_same(third, pareto_wide_ref.cut_to_keep(*full, 1), "third")


@pytest.mark.parametrize("Q,m", [(2048, 2), (2048, 3), (64, 2), (64, 8), (31, 3), (32, 3), (15, 8), (16, 8)])
def test_the_rule_with_a_workspace(Q, m):
    """Mode -1: whichever path the rule names (its thresholds are Q = 32 for m <= 4 and Q = 16 above; both sides of
    each are here), the result is the restatement's."""
    F = rank_input("gauss", Q, m)
    Fd = torch.from_numpy(F).to(DEV)
    for keep in (Q, Q // 2):
        with wide(-1):
            assert_same(device_rank(Fd, keep), pareto_ref.rank_crowd_order(F, keep), (Q, m, keep))


# ---------------------------------------------------------------- dkg_pareto_nsga2

GEN_NS = (20, 31, 16, 45, 27, 38, 18, 52)


@functools.lru_cache(maxsize=None)
def gen_model(d, m):
    state = grad_case(m, d, GEN_NS[:m], ALL_FAMILIES, 4, 2, 4, 100 * d + m)[0]
    g = np.random.default_rng(d + m)
    lb, ub = -0.25 - 0.5 * g.random(d), 1.0 + 0.5 * g.random(d)
    return PreparedModel(state, DEV), lb, ub


def manual_step(pm, lb, ub, X, F, rank, crowd, u):
    """One generation from the three stage entries; the glue (normalise, concatenate, gather) in torch."""
    lbt, ubt = torch.from_numpy(lb).to(DEV), torch.from_numpy(ub).to(DEV)
    C = pareto_variation(X, rank, crowd, lb, ub, u)
    FC = posterior_mean(pm, (C - lbt) / (ubt - lbt))
    X2, F2 = torch.cat([X, C]), torch.cat([F, FC])
    r2, c2, order = nondominated_rank(F2, X.shape[0])
    sel = order[:X.shape[0]].long()
    return X2[sel], F2[sel], r2[sel], c2[sel]


@pytest.mark.parametrize("P,d,m,gens", [(12, 2, 2, 3), (64, 3, 3, 3), (1024, 16, 8, 2)])
def test_nsga2_wide_against_one_workgroup(P, d, m, gens):
    pm, lb, ub = gen_model(d, m)
    u = torch.rand(P * d + gens * pareto_ref.draws(P, d), dtype=torch.double,
                   generator=torch.Generator().manual_seed(17 * P + d)).to(DEV)
    with wide(1):
        w = pareto_nsga2(pm, lb, ub, P, gens, u)
    with wide(0):
        n = pareto_nsga2(pm, lb, ub, P, gens, u)
    for a, b in zip(w, n):
        assert torch.equal(a, b) and bits(a) == bits(b)
    if P == 12:
        n0 = pareto_ref.draws(P, d)
        with wide(1):
            X, F, rank, crowd = pareto_nsga2(pm, lb, ub, P, 0, u)
            for g in range(gens):
                X, F, rank, crowd = manual_step(pm, lb, ub, X, F, rank, crowd, u[P * d + g * n0:P * d + (g + 1) * n0])
        for a, b in zip((X, F, rank, crowd), w):
            assert bits(a) == bits(b)


# ---------------------------------------------------------------- from Python

def test_nondominated_rank_beyond_2048_points_from_python():
    """Q = 4097 with no workspace argument: the call brings its own.  Before the wide path this raised
    UnsupportedError ("Q=4097 points (supported <= 2048)")."""
    F = rank_input("gauss", 4097, 3)
    rank, crowd, order = nondominated_rank(torch.from_numpy(F).to(DEV))
    assert rank.dtype == torch.int32 and crowd.dtype == torch.double and order.dtype == torch.int32
    assert_same((rank.cpu().numpy(), crowd.cpu().numpy(), order.cpu().numpy()), full_reference("gauss", 4097, 3),
                "Q=4097")
    r1 = nondominated_rank(F, keep=1, device=DEV)[0].cpu().numpy()
    assert r1.tolist() == pareto_wide_ref.cut_to_keep(*full_reference("gauss", 4097, 3), 1)[0].tolist()


def dominated_by(f, cand):
    """[len(f)] bool: some row of cand dominates the row of f (all maximised)."""
    ge = (cand[:, None, :] >= f[None, :, :]).all(-1)
    gt = (cand[:, None, :] > f[None, :, :]).any(-1)
    return (ge & gt).any(0)


def nondominated_mask(f, chunk=512):
    """mask[i]: no row of f dominates row i, without a Q x Q x m array.  Dominance is a strict partial order on a
    finite set, so a dominated row is dominated by a maximal row, and a maximal row survives any filter: first the
    rows no row of their own chunk dominates, then those of them no other survivor dominates."""
    Q = f.shape[0]
    keep = np.ones(Q, dtype=bool)
    for s in range(0, Q, chunk):
        keep[s:s + chunk] = ~dominated_by(f[s:s + chunk], f[s:s + chunk])
    alive = np.flatnonzero(keep)
    for s in range(0, alive.size, chunk):
        keep[alive[s:s + chunk]] = ~dominated_by(f[alive[s:s + chunk]], f[alive])
    return keep


def test_posterior_front_on_the_grid_of_the_golden_surrogate():
    """128 x 128 points of the unit square: the returned rows are exactly the device's own posterior-mean rows that
    no other row dominates, in index order (the reference is computed from the device's means: no tolerance)."""
    state, *_ = load_golden("lengthscales0")
    ax = np.linspace(0.0, 1.0, 128)
    G = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    assert G.shape == (MAXQ, 2)
    pm = PreparedModel(state, DEV)
    x, f = posterior_front_on_points(pm, G)
    mean = posterior_mean(pm, torch.from_numpy(G)).cpu().numpy()
    mask = nondominated_mask(mean)
    assert isinstance(x, np.ndarray) and isinstance(f, np.ndarray) and x.dtype == np.float64 and f.dtype == np.float64
    assert 0 < mask.sum() < MAXQ
    assert f.shape == (int(mask.sum()), 2) and f.tobytes() == np.ascontiguousarray(mean[mask]).tobytes()
    assert x.tobytes() == np.ascontiguousarray(G[mask]).tobytes()
    x2, f2 = posterior_front_on_points(state, G, device=DEV)  # a state: prepared inside the call
    assert x2.tobytes() == x.tobytes() and f2.tobytes() == f.tobytes()
