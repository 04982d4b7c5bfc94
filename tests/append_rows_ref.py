"""Host restatement (torch, fp64) of the block update of dkg_append_rows (include/dkg.h): the caches of
([X; X2], y') from those of (X, y) without refactorising.  Shared by test_append_rows_host.py, which checks it
against torch.linalg.cholesky of the augmented matrix, and by the GPU tests, which use its discretisation
columns."""

import torch

from dkg_amd.model import SingleTaskGPState
from oracle.gp import OutputGP


def covar(st: SingleTaskGPState, x1, x2):
    og = OutputGP(st.train_x, st.train_y, st.lengthscale, st.outputscale, st.noise, st.mean_constant, st.kernel,
                  st.nu)
    return og.covar(x1, x2)


def grown(st: SingleTaskGPState, X2, train_y) -> SingleTaskGPState:
    return SingleTaskGPState(torch.cat([st.train_x, X2]), train_y, st.lengthscale, st.outputscale, st.noise,
                             st.mean_constant, st.kernel, st.nu, st.y_mean, st.y_std)


def block_update(st: SingleTaskGPState, L, M, X2, train_y, jitter=0.0, D=None, QD=None):
    """st: the old output (n rows); L, M = L^{-1}: its factor and inverse; X2 [K, d]; train_y: all n + K targets.
    D [N, d] with QD = K(D, X) M^T adds the discretisation caches.  Returns a dict of L, M, alpha (and QD, muD)
    of the grown output, by the formulas of the header, or None when S is not positive definite."""
    n, K = st.num_train, X2.shape[0]
    c = float(st.mean_constant)
    r = train_y - c
    kx = covar(st, X2, st.train_x)                                   # s kappa(X2, X)
    B = kx @ M.T
    beta = M @ r[:n]
    S = covar(st, X2, X2) + (float(st.noise) + jitter) * torch.eye(K, dtype=torch.double) - B @ B.T
    C, info = torch.linalg.cholesky_ex(S)
    if int(info) != 0:
        return None
    Ci = torch.linalg.solve_triangular(C, torch.eye(K, dtype=torch.double), upper=False)
    W = B @ M
    n1 = n + K
    Ln = torch.zeros(n1, n1, dtype=torch.double)
    Mn = torch.zeros(n1, n1, dtype=torch.double)
    Ln[:n, :n], Ln[n:, :n], Ln[n:, n:] = L, B, C
    Mn[:n, :n], Mn[n:, :n], Mn[n:, n:] = M, -Ci @ W, Ci
    beta2 = Ci @ (r[n:] - B @ beta)
    gamma = Ci.T @ beta2
    alpha = torch.cat([M.T @ beta - W.T @ gamma, gamma])
    out = {"L": Ln, "M": Mn, "alpha": alpha}
    if D is not None:
        new = (covar(st, D, X2) - QD @ B.T) @ Ci.T
        out["QD"] = torch.cat([QD, new], dim=1)
        out["muD"] = c + QD @ beta + new @ beta2
    return out


def dense_from_frag(frag, rows: int, n: int):
    """The dense [pad16(rows), pad16(n)] matrix of a fragment-packed one (include/dkg.h "Data layout":
    F[t][j][l][h] = P[16 t + (l & 15)][4 (2 j + h) + (l >> 4)])."""
    rp, np_ = (rows + 15) // 16 * 16, (n + 15) // 16 * 16
    F = frag[: rp * np_].reshape(rp // 16, np_ // 8, 64, 2)
    t = torch.arange(rp // 16).reshape(-1, 1, 1, 1)
    j = torch.arange(np_ // 8).reshape(1, -1, 1, 1)
    l = torch.arange(64).reshape(1, 1, -1, 1)
    h = torch.arange(2).reshape(1, 1, 1, -1)
    row = (16 * t + (l & 15)).expand_as(F)
    col = (4 * (2 * j + h) + (l >> 4)).expand_as(F)
    out = torch.empty(rp, np_, dtype=frag.dtype)
    out[row.reshape(-1), col.reshape(-1)] = F.reshape(-1)
    return out
