"""Numpy restatement of the JES Pareto sampler (include/dkg.h "The Pareto samples of joint entropy search"): test
infrastructure, not a test.  Every function follows the header's specification, not the device code; the generations
are tests/pareto_ref.py's.

* ``omega_bias`` / ``features``: the random Fourier feature map of one output;
* ``weights``: the weight-space posterior sample of every (sample, output) (``dkg_rff_weights``);
* ``evaluate`` / ``evaluate_longdouble``: the paths at points (``dkg_rff_eval``), the second in extended precision
  with the magnitudes a rounding model needs;
* ``kernel``: the covariance the feature map approximates;
* ``prune``: ``dkg_pareto_prune`` in plain loops;
* ``run``: the evolution of one sample (``dkg_pareto_nsga2_paths``) through ``pareto_ref.run``.
"""

import numpy as np

import pareto_ref

TWO_PI = 2.0 * np.pi
MATERN_NU = {0: 0.5, 1: 1.5, 2: 2.5}  # enum dkg_kernel -> nu; 3 is DKG_RBF


def kernel_id(st):
    return 3 if st.kernel == "rbf" else {0.5: 0, 1.5: 1, 2.5: 2}[float(st.nu)]


def omega_bias(wn, g, ub, inv_ls, kid):
    """omega [R, d] and bias [R] of one (sample, output) from its draws."""
    om = np.asarray(wn, dtype=np.float64) * np.asarray(inv_ls, dtype=np.float64)
    if kid != 3:
        om = om * (1.0 / np.sqrt(np.asarray(g, dtype=np.float64)))[:, None]
    return om, TWO_PI * np.asarray(ub, dtype=np.float64)


def features(x, om, b, s):
    """Phi [k, R] = sqrt(2 s / R) cos(x omega^T + b)."""
    return np.sqrt(2.0 * s / om.shape[0]) * np.cos(np.asarray(x, dtype=np.float64) @ om.T + b)


def kernel(x1, x2, inv_ls, kid):
    """kappa(x1_i, x2_j) of the family ``kid`` (unit outputscale)."""
    t = (np.asarray(x1)[:, None, :] - np.asarray(x2)[None, :, :]) * inv_ls
    r2 = (t * t).sum(-1)
    if kid == 3:
        return np.exp(-0.5 * r2)
    a = np.sqrt(2.0 * MATERN_NU[kid]) * np.sqrt(r2)
    poly = {0: 1.0, 1: 1.0 + a, 2: 1.0 + a + 5.0 / 3.0 * r2}[kid]
    return poly * np.exp(-a)


def weights(state, wn, g, ub, z, reverse_rows=False):
    """-> dict(omega [S, m, R, d], bias, coef [S, m, R], offset [S, m]) for the model ``state`` (a ModelListGPState)
    and draws of the shapes of ``dkg_amd.jes_pareto.draw_rff_randomness``.  ``reverse_rows``: the training rows in
    reverse order (the same sample in exact arithmetic: the spread of the two is the restatement's own rounding
    floor)."""
    wn, g, ub, z = (np.asarray(t, dtype=np.float64) for t in (wn, g, ub, z))
    S, m, R, d = wn.shape
    out = dict(omega=np.empty((S, m, R, d)), bias=np.empty((S, m, R)), coef=np.empty((S, m, R)),
               offset=np.empty((S, m)))
    for i, st in enumerate(state.models):
        X = st.train_x.numpy()
        y = st.train_y.numpy()
        if reverse_rows:
            X, y = X[::-1], y[::-1]
        kid = kernel_id(st)
        inv_ls = 1.0 / st.lengthscale.numpy()
        s, noise, c = float(st.outputscale), float(st.noise), float(st.mean_constant)
        amp = np.sqrt(2.0 * s / R)
        for k in range(S):
            om, b = omega_bias(wn[k, i], g[k, i], ub[k, i], inv_ls, kid)
            Phi = features(X, om, b, s)
            A = Phi.T @ Phi + noise * np.eye(R)
            L = np.linalg.cholesky(A)
            t = np.linalg.solve(L, Phi.T @ (y - c)) + np.sqrt(noise) * z[k, i]
            theta = np.linalg.solve(L.T, t)
            out["omega"][k, i], out["bias"][k, i] = om, b
            out["coef"][k, i] = float(st.y_std) * amp * theta
            out["offset"][k, i] = float(st.y_mean) + float(st.y_std) * c
    return out


def evaluate(paths, X):
    """F [S, P, m] of X [P, d] (shared) or [S, P, d]."""
    om, b, co, off = (np.asarray(paths[k]) for k in ("omega", "bias", "coef", "offset"))
    S, m = off.shape
    X = np.asarray(X, dtype=np.float64)
    Xs = np.broadcast_to(X, (S,) + X.shape[-2:])
    F = np.empty((S, Xs.shape[1], m))
    for s in range(S):
        for i in range(m):
            F[s, :, i] = off[s, i] + np.cos(Xs[s] @ om[s, i].T + b[s, i]) @ co[s, i]
    return F


def evaluate_longdouble(paths, X):
    """-> (F [S, P, m] in extended precision, bound [S, P, m] float64): the rounding model of dkg_rff_eval with
    u = 2^-53.  Per feature the device's phase is d fmas and the addition of b_r, so it is off by at most
    (d + 1) u (|b_r| + sum_j |omega_rj x_j|) =: dphi_r (each partial sum is bounded by that magnitude), and cos moves
    by at most dphi_r plus the 2 ulp of the device's cos; the lane chain has ceil(R / 64) fmas and the wave
    reduction 6 additions, then the offset's one: (ceil(R / 64) + 7) u sum_r |coef_r|, and u |F| for the last
    rounding of the magnitude of the result.  First order; the factor 2 covers the higher-order terms."""
    ld = np.longdouble
    u = 2.0 ** -53
    om, b, co, off = (np.asarray(paths[k]) for k in ("omega", "bias", "coef", "offset"))
    S, m, R, d = om.shape
    X = np.asarray(X, dtype=np.float64)
    Xs = np.broadcast_to(X, (S,) + X.shape[-2:])
    P = Xs.shape[1]
    F = np.empty((S, P, m), dtype=ld)
    bound = np.empty((S, P, m))
    for s in range(S):
        xl = Xs[s].astype(ld)
        for i in range(m):
            ph = xl @ om[s, i].astype(ld).T + b[s, i].astype(ld)
            F[s, :, i] = off[s, i].astype(ld) + np.cos(ph) @ co[s, i].astype(ld)
            mag = np.abs(b[s, i])[None, :] + np.abs(Xs[s]) @ np.abs(om[s, i]).T  # [P, R]
            dphi = (d + 1) * u * mag
            ac = np.abs(co[s, i])
            bound[s, :, i] = 2.0 * ((dphi + 4 * u) @ ac + (-(-R // 64) + 7) * u * ac.sum()
                                    + u * np.abs(F[s, :, i]).astype(np.float64))
    return F, bound


def crowding(F):
    """dkg_pareto_rank's crowding of one front F [k, m] (every row a member)."""
    k, m = F.shape
    cd = np.zeros(k)
    with np.errstate(all="ignore"):
        for j in range(m):
            srt = np.lexsort((np.arange(k), F[:, j]))
            cd[srt[0]] = cd[srt[0]] + np.inf
            cd[srt[-1]] = cd[srt[-1]] + np.inf
            if k > 2:
                rng = F[srt[-1], j] - F[srt[0], j]
                num = F[srt[2:], j] - F[srt[:-2], j]
                cd[srt[1:-1]] = cd[srt[1:-1]] + (num / rng if rng > 0.0 else np.zeros_like(num))
    return cd


def prune(F, rank, k):
    """dkg_pareto_prune of one sample: F [Q, m], rank [Q] -> the indices that stay, ascending."""
    F = np.asarray(F, dtype=np.float64)
    Q = F.shape[0]
    alive = [i for i in range(Q) if rank[i] == 0]
    keep = []
    for i in alive:  # of bit-equal objective vectors the lowest index stays
        if not any(F[j].tobytes() == F[i].tobytes() for j in keep):
            keep.append(i)
    while len(keep) > k:
        cd = crowding(F[keep])
        worst = min(range(len(keep)), key=lambda a: (cd[a], keep[a]))
        del keep[worst]
    return keep


def fitness(paths, s, lb=None, ub=None):
    """pareto_ref.run's fitness for sample s: the path at the points normalised with lb / ub when given."""
    one = {k: np.asarray(v)[s:s + 1] for k, v in paths.items()}
    if lb is None:
        return lambda X: evaluate(one, X)[0]
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    return lambda X: evaluate(one, (X - lb) / (ub - lb))[0]


def run(paths, s, lb, ub, P, gens, u, **prm):
    """dkg_pareto_nsga2_paths for sample s from its row of uniforms: (X, F, rank, crowd)."""
    return pareto_ref.run(fitness(paths, s, lb, ub), lb, ub, P, gens, u, **prm)
