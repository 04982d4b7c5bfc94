"""Numpy restatement of the device NSGA-II (include/dkg.h "Posterior-mean Pareto front"): test infrastructure,
not a test.  Every function follows the header's specification, not the device code:

* ``rank_crowd_order``: dominance, the front peel, crowding and the survivor order (``dkg_pareto_rank``);
* ``variation``: tournament, bounded SBX, bounded polynomial mutation from the same uniforms
  (``dkg_pareto_variation``; libm's ``pow`` against the device's, so children agree to a few ulp of the terms);
* ``survive`` / ``step``: one generation's (mu + lambda) survival;
* ``run``: a whole evolution (``dkg_pareto_nsga2``) with any fitness; ``oracle_fitness`` is ``oracle.gp``'s
  posterior mean;
* ``hypervolume_2d``: the exact dominated area (m = 2), for the quality yardstick.
"""

import numpy as np

DEFAULTS = dict(cr=0.95, eta_c=10.0, m=0.01, eta_m=50.0)  # pygmo.nsga2's documented defaults


def dominance_matrix(F):
    """dom[k, i]: point k dominates point i (all maximised; equal points do not dominate each other)."""
    F = np.asarray(F, dtype=np.float64)
    ge = (F[:, None, :] >= F[None, :, :]).all(-1)
    gt = (F[:, None, :] > F[None, :, :]).any(-1)
    return ge & gt


def rank_crowd_order(F, keep=None):
    """-> (rank int32 [Q], crowd float64 [Q], order int32 [Q]) as dkg_pareto_rank specifies them."""
    F = np.asarray(F, dtype=np.float64)
    Q, m = F.shape
    keep = Q if keep is None else int(keep)
    dom = dominance_matrix(F)
    cnt = dom.sum(0).astype(np.int64)
    rank = np.full(Q, -1, dtype=np.int32)
    done, r = 0, 0
    while done < keep and r < Q:
        front = np.flatnonzero((rank < 0) & (cnt == 0))
        if front.size == 0:
            break
        rank[front] = r
        cnt[front] = -1
        cnt -= np.where(rank < 0, dom[front].sum(0), 0)
        done += front.size
        r += 1
    crowd = np.zeros(Q, dtype=np.float64)
    with np.errstate(all="ignore"):
        for fr in range(r):
            members = np.flatnonzero(rank == fr)
            for j in range(m):
                fj = F[members, j]
                srt = members[np.lexsort((members, fj))]  # (f_j ascending, index ascending)
                crowd[srt[0]] = crowd[srt[0]] + np.inf
                crowd[srt[-1]] = crowd[srt[-1]] + np.inf
                if srt.size > 2:
                    rng = F[srt[-1], j] - F[srt[0], j]
                    num = F[srt[2:], j] - F[srt[:-2], j]
                    add = num / rng if rng > 0.0 else np.zeros_like(num)
                    crowd[srt[1:-1]] = crowd[srt[1:-1]] + add
    ranked = np.flatnonzero(rank >= 0)
    srt = ranked[np.lexsort((ranked, -crowd[ranked], rank[ranked]))]
    order = np.full(Q, -1, dtype=np.int32)
    order[:srt.size] = srt
    return rank, crowd, order


def draws(P, d):
    """dkg_pareto_draws."""
    H = P // 2
    return 2 * P + H + 3 * H * d + 2 * P * d


def tournament_winners(rank, crowd, u, P):
    t = np.asarray(u[:2 * P], dtype=np.float64).reshape(P, 2)
    i0 = np.clip((t[:, 0] * P).astype(np.int64), 0, P - 1)
    i1 = np.clip((t[:, 1] * P).astype(np.int64), 0, P - 1)
    second = (rank[i1] < rank[i0]) | ((rank[i1] == rank[i0]) & (crowd[i1] > crowd[i0]))
    return np.where(second, i1, i0)


def _betaq(u, beta, eta):
    alpha = 2.0 - np.power(beta, -(eta + 1.0))
    e = 1.0 / (eta + 1.0)
    return np.where(u <= 1.0 / alpha, np.power(u * alpha, e), np.power(1.0 / (2.0 - u * alpha), e))


def _poly_mutate(y, lb, ub, u, eta):
    span = ub - lb
    d1, d2 = (y - lb) / span, (ub - y) / span
    mp = 1.0 / (eta + 1.0)
    lo_val = 2.0 * u + (1.0 - 2.0 * u) * np.power(1.0 - d1, eta + 1.0)
    hi_val = 2.0 * (1.0 - u) + 2.0 * (u - 0.5) * np.power(1.0 - d2, eta + 1.0)
    dq = np.where(u < 0.5, np.power(lo_val, mp) - 1.0, 1.0 - np.power(hi_val, mp))
    return np.where(span > 0.0, np.clip(y + dq * span, lb, ub), y)


def variation(X, rank, crowd, lb, ub, u, cr=0.95, eta_c=10.0, m=0.01, eta_m=50.0):
    """P children of the ranked population X from the uniforms u (layout: include/dkg.h, dkg_pareto_draws)."""
    X = np.asarray(X, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    P, d = X.shape
    H = P // 2
    W = X[tournament_winners(rank, crowd, u, P)]
    c0, c1 = W[0::2].copy(), W[1::2].copy()
    gate = u[2 * P:2 * P + H] < cr
    ux = u[2 * P + H:2 * P + H + 3 * H * d].reshape(H, d, 3)
    y1, y2 = np.minimum(c0, c1), np.maximum(c0, c1)
    dy = y2 - y1
    do = gate[:, None] & (ux[..., 0] < 0.5) & (dy > 1e-14)
    with np.errstate(all="ignore"):
        sdy = np.where(do, dy, 1.0)
        bq1 = _betaq(ux[..., 1], 1.0 + 2.0 * (y1 - lb) / sdy, eta_c)
        bq2 = _betaq(ux[..., 1], 1.0 + 2.0 * (ub - y2) / sdy, eta_c)
        n1 = np.clip(0.5 * ((y1 + y2) - bq1 * dy), lb, ub)
        n2 = np.clip(0.5 * ((y1 + y2) + bq2 * dy), lb, ub)
        swap = ux[..., 2] < 0.5
        c0 = np.where(do, np.where(swap, n2, n1), c0)
        c1 = np.where(do, np.where(swap, n1, n2), c1)
        C = np.empty_like(X)
        C[0::2], C[1::2] = c0, c1
        um = u[2 * P + H + 3 * H * d:2 * P + H + 3 * H * d + 2 * P * d].reshape(P, d, 2)
        C = np.where(um[..., 0] < m, _poly_mutate(C, lb, ub, um[..., 1], eta_m), C)
    return np.clip(C, lb, ub)


def survive(X2, F2, keep):
    """The survivors of [parents; children] in order order: (X, F, rank, crowd, order)."""
    rank, crowd, order = rank_crowd_order(F2, keep)
    sel = order[:keep]
    return X2[sel], F2[sel], rank[sel], crowd[sel], order


def step(X, F, rank, crowd, lb, ub, u, fitness, **prm):
    """One generation: variation, fitness of the children, survival of the 2P points with keep = P."""
    C = variation(X, rank, crowd, lb, ub, u, **prm)
    FC = fitness(C)
    return survive(np.concatenate([X, C]), np.concatenate([F, FC]), X.shape[0])[:4]


def run(fitness, lb, ub, P, gens, u, history=None, **prm):
    """dkg_pareto_nsga2: (X, F, rank, crowd) after ``gens`` generations; ``history`` (a list) receives a copy of
    (X, F, rank) after generation 0 and after every later one."""
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    d = lb.size
    u = np.asarray(u, dtype=np.float64)
    X = np.clip(lb + u[:P * d].reshape(P, d) * (ub - lb), lb, ub)
    F = fitness(X)
    rank, crowd, _ = rank_crowd_order(F, P)
    if history is not None:
        history.append((X.copy(), F.copy(), rank.copy()))
    n = draws(P, d)
    for g in range(gens):
        X, F, rank, crowd = step(X, F, rank, crowd, lb, ub, u[P * d + g * n:P * d + (g + 1) * n], fitness, **prm)
        if history is not None:
            history.append((X.copy(), F.copy(), rank.copy()))
    return X, F, rank, crowd


def oracle_mean(om, X):
    """oracle.gp's posterior mean of every output at X [P, d] (numpy in, numpy out), without the covariance."""
    import torch

    Xt = torch.as_tensor(np.asarray(X), dtype=torch.double)
    cols = [((o.covar(Xt, o.train_x) @ o.cache()["alpha"] + o.mean_constant) * o.y_std + o.y_mean) for o in om.models]
    return torch.stack(cols, dim=-1).numpy()


def oracle_fitness(om, lb=None, ub=None):
    """The fitness of ``run``: the oracle mean, of the points normalised with lb / ub when they are given
    (a surrogate, sample.py:129-130), else of the points as they are (a test problem)."""
    if lb is None:
        return lambda X: oracle_mean(om, X)
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    return lambda X: oracle_mean(om, (X - lb) / (ub - lb))


def uniforms(seed, P, d, gens):
    """The uniforms dkg_amd.pareto draws for (seed, P, d, gens): a CPU torch.Generator of its own."""
    import torch

    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.rand(P * d + gens * draws(P, d), dtype=torch.double, generator=g).numpy()


def hypervolume_2d(F, ref):
    """Exact area dominated by the points F [n, 2] above ref (maximisation); points not above ref add nothing."""
    F = np.asarray(F, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    F = F[(F > ref).all(-1)]
    if F.shape[0] == 0:
        return 0.0
    F = F[np.lexsort((-F[:, 1], -F[:, 0]))]  # f0 descending
    hv, best1 = 0.0, ref[1]
    for f0, f1 in F:
        if f1 > best1:
            hv += (f0 - ref[0]) * (f1 - best1)
            best1 = f1
    return float(hv)
