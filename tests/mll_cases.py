"""The case matrix and the yardstick of the marginal log-likelihood tests (dkg_mll_value_grad, dkg_amd.fit's
device objective): shared by tests/test_mll_oracle.py (CPU) and tests/test_gpu_mll.py.

Yardstick: a difference-form fp64 torch restatement of log N(y | c 1, s kappa(X, X) + (noise + jitter) I) with
autograd for the gradient in (c, lengthscales, s, noise).  Scaled distances come from the differences
(x_i - x_k) / l, as the device kernels take them (scaled_r2), with fit.matern's clamp (r^2 at 1e-30 before the
square root); fit.matern itself expands |a|^2 + |b|^2 - 2 a.b, which moves a Matern-1/2 gradient by up to 1e-6
of max|g|, so fit._Output.mll is not the yardstick.

Data: drawn from the GP itself (as tests/test_fit.py::_data), and evaluated 10-30 % away from the generating
hyperparameters, so no gradient component is near zero by accident.  The shapes are the smallest at which the
kernel can still go wrong: one tile (n = 1), the pad boundary (15, 16, 17), two Cholesky blocks (33), 100, across
128 (130), 272, and once the `once` path's 1000; d = 1, 2, 6, 16; the four families; noise 1e-4 and 1e-2; a
non-zero mean everywhere.  Everything is computed once per process and shared (functools.lru_cache)."""

import functools
import math

import numpy as np
import torch

NU = {"m12": 0.5, "m32": 1.5, "m52": 2.5, "rbf": math.inf}
KERNEL_ID = {"m12": 0, "m32": 1, "m52": 2, "rbf": 3}


def out(n, d, fam, noise, seed, dup=False, os=2.0):
    return dict(n=n, d=d, fam=fam, noise=noise, seed=seed, dup=dup, os=os)


# name -> (outputs, the absolute jitter the factorisation is expected to need)
CASES = {
    "n1_m52_d2": ([out(1, 2, "m52", 1e-2, 1)], 0.0),
    "n15_m12_d1": ([out(15, 1, "m12", 1e-4, 2)], 0.0),
    "n16_m32_d2": ([out(16, 2, "m32", 1e-2, 3)], 0.0),
    "n16_m12_d16": ([out(16, 16, "m12", 1e-4, 4)], 0.0),
    "n17_rbf_d6": ([out(17, 6, "rbf", 1e-4, 5)], 0.0),
    "n17_m32_d1": ([out(17, 1, "m32", 1e-2, 6)], 0.0),
    "n33_m52_d16": ([out(33, 16, "m52", 1e-2, 7)], 0.0),
    "n33_rbf_d2": ([out(33, 2, "rbf", 1e-2, 8)], 0.0),
    "n100_m12_d2": ([out(100, 2, "m12", 1e-2, 9)], 0.0),
    "n100_rbf_d2": ([out(100, 2, "rbf", 1e-4, 10)], 0.0),
    "n100_m32_d16": ([out(100, 16, "m32", 1e-4, 11)], 0.0),
    "n130_m32_d6": ([out(130, 6, "m32", 1e-4, 12)], 0.0),
    "n130_m52_d1": ([out(130, 1, "m52", 1e-4, 13)], 0.0),
    "n272_rbf_d1": ([out(272, 1, "rbf", 1e-2, 14)], 0.0),
    "n272_m52_d16": ([out(272, 16, "m52", 1e-4, 15)], 0.0),
    "n1000_m52_d2": ([out(1000, 2, "m52", 1e-4, 16)], 0.0),
    # two training points duplicated: r = 0 off the diagonal (Matern-1/2: h = 0 there, the clamp's gradient)
    "dup_m12": ([out(40, 2, "m12", 1e-2, 17, dup=True)], 0.0),
    "dup_m52": ([out(40, 2, "m52", 1e-4, 31, dup=True)], 0.0),
    # one call, unequal n and mixed families; eight outputs at the pad boundary
    "m3_mixed": ([out(17, 2, "m12", 1e-2, 19), out(130, 2, "rbf", 1e-4, 20), out(64, 2, "m32", 1e-2, 21)], 0.0),
    "m8_n16": ([out(16, 2, fam, noise, 22 + i) for i, (fam, noise) in enumerate(
        [("m12", 1e-4), ("m32", 1e-2), ("m52", 1e-4), ("rbf", 1e-2)] * 2)], 0.0),
    # needs the first jitter retry: RBF with a duplicated point and a noise of -2e-9, so K has the eigenvalue -2e-9
    # (the duplicated pair's difference) and no rounding makes it factor; noise 0 is not enough -- the pivots of a
    # numerically singular RBF matrix come out positive or not by rounding alone, and the device factored it.  The
    # outputscale is 1e-6, so the jitter 1e-8 leaves a well conditioned matrix (~n s / 8e-9) and the comparison at
    # that jitter is as sharp as elsewhere.
    "jitter_rbf": ([out(48, 2, "rbf", -2e-9, 30, dup=True, os=1e-6)], 1e-8),
}
SINGLE = [k for k, (o, _) in CASES.items() if len(o) == 1]

# The yardstick's own spread: the worst |autograd - numpy W-contraction|_inf / max|g| over the cases, measured by
# tests/test_mll_oracle.py (which asserts it stays under 1e-9) -- 3.3e-10, at n = 1000; 1.1e-10 at n = 130 (Matern-5/2,
# d = 1, noise 1e-4) is the worst of the others; the values agree to 3.1e-12 relative.  The device tolerance is 100
# times that (its ~1-ulp exp / sqrt variants and its own summation order), capped at 1e-8: the cap binds.
CPU_SPREAD = 3.4e-10
CPU_VALUE_SPREAD = 3.1e-12
TOL = min(100.0 * CPU_SPREAD, 1e-8)
VALUE_TOL = min(100.0 * CPU_VALUE_SPREAD, 1e-8)  # the same rule on the value's relative error
FLOOR = 1e3 * TOL  # of max|g|: what a gradient component must exceed (on >= 90 % of the rows) to be pinned


def kernel_torch(X, ls, nu):
    """kappa(|(x - x') / l|) from the differences, r^2 clamped at 1e-30 as fit.matern does."""
    Z = X / ls
    diff = Z[:, None, :] - Z[None, :, :]
    r2 = (diff * diff).sum(-1).clamp_min(1e-30)
    if math.isinf(nu):
        return torch.exp(-0.5 * r2)
    r = r2.sqrt()
    if nu == 0.5:
        return torch.exp(-r)
    if nu == 1.5:
        t = math.sqrt(3.0) * r
        return (1.0 + t) * torch.exp(-t)
    t = math.sqrt(5.0) * r
    return (1.0 + t + t * t / 3.0) * torch.exp(-t)


def log_lik(X, y, nu, c, ls, s, noise, jitter=0.0):
    n = X.shape[0]
    K = s * kernel_torch(X, ls, nu) + (noise + jitter) * torch.eye(n, dtype=torch.double)
    L = torch.linalg.cholesky(K)
    a = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False)
    return -0.5 * (a * a).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def data(name):
    """Per output: X [n, d], y [n], nu and the evaluation point (mean, lengthscales [d], outputscale, noise)."""
    outs, jitter = CASES[name]
    res = []
    for o in outs:
        n, d = o["n"], o["d"]
        g = torch.Generator().manual_seed(1000 + o["seed"])
        X = torch.rand(n, d, generator=g, dtype=torch.double)
        if o["dup"]:
            X[n // 2] = X[3]
        ls_gen = torch.tensor([(0.25 + 0.2 * (j % 3)) * math.sqrt(d) for j in range(d)], dtype=torch.double)
        os_gen, mean_gen = o["os"], 0.3 * math.sqrt(o["os"])
        noise_gen = max(o["noise"] / 1.2, 1e-6 * os_gen, jitter)
        Kg = os_gen * kernel_torch(X, ls_gen, NU[o["fam"]]) + noise_gen * torch.eye(n, dtype=torch.double)
        y = mean_gen + torch.linalg.cholesky(Kg) @ torch.randn(n, generator=g, dtype=torch.double)
        if o["dup"] and o["noise"] <= 0.0:
            y[n // 2] = y[3]
        sign = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(d)], dtype=torch.double)
        frac = torch.tensor([0.12 + 0.03 * (j % 6) for j in range(d)], dtype=torch.double)
        res.append(dict(X=X, y=y, fam=o["fam"], nu=NU[o["fam"]], mean=mean_gen + 0.25 * math.sqrt(os_gen),
                        ls=ls_gen * (1.0 + sign * frac), os=os_gen * 1.2, noise=o["noise"]))
    return res


def hyper_of(name):
    ds = data(name)
    return {"means": [o["mean"] for o in ds], "length_scales": [o["ls"].tolist() for o in ds],
            "output_scales": [o["os"] for o in ds], "noises": [o["noise"] for o in ds]}


def config_of(name):
    """The model_config["outputs"] entries fit.mll_value_and_grad reads the families from."""
    return {"outputs": [{"kernel": {"type": "rbf"} if o["fam"] == "rbf" else
                         {"type": "matern", "args": {"nu": o["nu"]}}} for o in data(name)]}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The yardstick: (values [m], grads [m][d + 3] = [mean, lengthscales, outputscale, noise]) by autograd, at
    the case's jitter."""
    jitter = CASES[name][1]
    vals, grads = [], []
    for o in data(name):
        p = [torch.tensor(o["mean"], dtype=torch.double, requires_grad=True), o["ls"].clone().requires_grad_(True),
             torch.tensor(o["os"], dtype=torch.double, requires_grad=True),
             torch.tensor(o["noise"], dtype=torch.double, requires_grad=True)]
        v = log_lik(o["X"], o["y"], o["nu"], p[0], p[1], p[2], p[3], jitter)
        g = torch.autograd.grad(v, p)
        vals.append(float(v.detach()))
        grads.append(np.concatenate([np.atleast_1d(t.numpy()) for t in g]))
    return np.array(vals), grads


def _profile_np(fam, r2):
    """(kappa, h = kappa'(r) / r) of a family at squared scaled distances r2 (h: 0 for Matern-1/2 at r2 <= 1e-30)."""
    if fam == "rbf":
        k = np.exp(-0.5 * r2)
        return k, -k
    r = np.sqrt(r2)
    if fam == "m12":
        k = np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(r2 > 1e-30, -k / np.where(r2 > 1e-30, r, 1.0), 0.0)
        return k, h
    if fam == "m32":
        t = math.sqrt(3.0) * r
        return (1.0 + t) * np.exp(-t), -3.0 * np.exp(-t)
    t = math.sqrt(5.0) * r
    return (1.0 + t + t * t / 3.0) * np.exp(-t), -(5.0 / 3.0) * (1.0 + t) * np.exp(-t)


@functools.lru_cache(maxsize=None)
def numpy_reference(name):
    """A second, independent fp64 evaluation: numpy, explicit L^{-1}, and the W-contraction formulas the device
    uses (include/dkg.h, dkg_mll_value_grad)."""
    from scipy.linalg import cholesky, solve_triangular

    jitter = CASES[name][1]
    vals, grads = [], []
    for o in data(name):
        X, y, ls = o["X"].numpy(), o["y"].numpy(), o["ls"].numpy()
        n, d = X.shape
        T = (X[:, None, :] - X[None, :, :]) / ls
        T2 = T * T
        kap, h = _profile_np(o["fam"], T2.sum(-1))
        K = o["os"] * kap + (o["noise"] + jitter) * np.eye(n)
        L = cholesky(K, lower=True)
        M = solve_triangular(L, np.eye(n), lower=True)
        r = y - o["mean"]
        alpha = M.T @ (M @ r)
        W = np.outer(alpha, alpha) - M.T @ M
        vals.append(-0.5 * r @ alpha - np.log(np.diag(L)).sum() - 0.5 * n * math.log(2.0 * math.pi))
        g_ls = [-0.5 * o["os"] * (W * h * T2[:, :, j]).sum() / ls[j] for j in range(d)]
        grads.append(np.array([alpha.sum()] + g_ls + [0.5 * (W * kap).sum(), 0.5 * np.trace(W)]))
    return np.array(vals), grads
