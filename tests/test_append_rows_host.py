"""The host side of the block update (dkg_append_rows, include/dkg.h): the declarations, the ctypes layout, the
argument checks, which come before any HIP call and so need no GPU, and the host restatement of the update
(append_rows_ref.block_update) against torch.linalg.cholesky of the augmented matrix."""

import ctypes
import os
import re

import pytest
import torch

from append_rows_ref import block_update, covar, grown
from dkg_amd import _lib
from dkg_amd.model import SingleTaskGPState

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dkg.h")


def test_header_declares_the_block_update():
    text = open(HEADER).read()
    assert re.search(r"#define\s+DKG_APPEND_MAX_ROWS\s+32\b", text)
    assert re.search(r"#define\s+DKG_APPEND_MAX_JOBS\s+512\b", text)
    assert "typedef struct dkg_append_job {" in text and "} dkg_append_job;" in text
    assert "size_t dkg_append_rows_workspace(const dkg_append_job* jobs, int J, int d);" in text
    assert re.search(r"int dkg_append_rows\(const dkg_append_job\* jobs, int J, int d, int32_t\* info", text)
    assert re.search(r"#define\s+DKG_ABI_VERSION\s+9\b", text)
    lib = _lib.load()
    assert lib.dkg_abi_version() == 9 and _lib.ABI_VERSION == 9
    for name in ("dkg_append_rows", "dkg_append_rows_workspace"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert (_lib.DKG_APPEND_MAX_ROWS, _lib.DKG_APPEND_MAX_JOBS) == (32, 512)
    assert _lib.DKG_APPEND_MAX_JOBS == _lib.DKG_JES_MAX_SAMPLES * _lib.MAX_OUTPUTS


def test_struct_layout_matches_header():
    """The header's member order; every member at its natural alignment (the two int32 share a word)."""
    J = _lib.DkgAppendJob
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct dkg_append_job \{(.*?)\} dkg_append_job;", text, flags=re.S).group(1)
    names = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
    assert names == [f[0] for f in J._fields_]
    assert ctypes.sizeof(J) == 4 * 8 + 2 * 4 + 2 * 8 + 8 + 6 * 8
    offsets = {f[0]: getattr(J, f[0]).offset for f in J._fields_}
    assert offsets["o"] == 0 and offsets["disc"] == 24 and offsets["N"] == 32 and offsets["K"] == 36
    assert offsets["train_x"] == 40 and offsets["jitter"] == 56 and offsets["L_new"] == 64
    assert offsets["disc_mean_new"] == 104


# --------------------------------------------------------------------------------------------------
# argument checks: no device call is reached

def fake_output(n):
    o = _lib.DkgOutput()
    o.n = n
    o.kernel = 2
    o.outputscale, o.noise, o.y_std = 1.0, 1e-3, 1.0
    for f in ("inv_lengthscale", "train_x", "alpha", "root_frag", "disc_frag", "disc_mean"):
        setattr(o, f, 64)  # never dereferenced: the checks come first
    return o


def fake_jobs(J=1, n=64, K=3, N=16, **kw):
    outs = [fake_output(n) for _ in range(J)]
    jobs = (_lib.DkgAppendJob * max(J, 1))()
    for j in range(J):
        b = jobs[j]
        b.o = ctypes.pointer(outs[j])
        b.N, b.K, b.jitter = N, K, 0.0
        for f in ("L", "Linv", "disc", "train_x", "train_y", "L_new", "Linv_new", "alpha_new", "root_frag_new",
                  "disc_frag_new", "disc_mean_new"):
            setattr(b, f, 64)
        for k, v in kw.items():
            setattr(b, k, v)
    jobs._keep = outs
    return jobs


def run(jobs, J, d=2, work=64, work_bytes=1 << 40):
    lib = _lib.load()
    info = (ctypes.c_int32 * max(J, 1))()
    st = lib.dkg_append_rows(jobs, J, d, info, work, work_bytes, None)
    return st, lib.dkg_last_error().decode()


def test_job_count():
    assert run(fake_jobs(1), 0) == (_lib.DKG_ERR_ARG, "J=0 jobs")
    assert run(fake_jobs(513), 513) == (_lib.DKG_ERR_UNSUPPORTED, "J=513 jobs (supported 1..512)")
    assert run(None, 1) == (_lib.DKG_ERR_ARG, "jobs is NULL")
    lib = _lib.load()
    assert lib.dkg_append_rows(fake_jobs(1), 1, 2, None, 64, 1 << 40, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_last_error() == b"info is NULL"


def test_row_count():
    assert run(fake_jobs(2, K=0), 2) == (_lib.DKG_ERR_ARG, "job 0: K=0 new rows")
    assert run(fake_jobs(1, K=33), 1) == (_lib.DKG_ERR_UNSUPPORTED, "job 0: K=33 new rows (supported 1..32)")
    assert run(fake_jobs(1, K=32), 1, work_bytes=0)[0] == _lib.DKG_ERR_WORKSPACE  # K = 32 itself passes the checks


def test_beyond_1024_training_points():
    assert run(fake_jobs(1, n=1000, K=32), 1) == (_lib.DKG_ERR_UNSUPPORTED, "job 0: n=1032 > 1024 training points")
    assert run(fake_jobs(1, n=992, K=32), 1, work_bytes=0)[0] == _lib.DKG_ERR_WORKSPACE  # n = 1024 is supported


def test_null_pointers():
    assert run(fake_jobs(3, L_new=None), 3) == (_lib.DKG_ERR_ARG, "job 0: NULL pointer")
    for name in ("L", "Linv", "train_x", "train_y", "Linv_new", "alpha_new", "root_frag_new"):
        assert run(fake_jobs(1, **{name: None}), 1) == (_lib.DKG_ERR_ARG, "job 0: NULL pointer"), name
    assert run(fake_jobs(1, disc=None), 1) == (_lib.DKG_ERR_ARG, "job 0: N=16 with a NULL discretisation pointer")
    assert run(fake_jobs(1, N=0, disc=None, disc_frag_new=None, disc_mean_new=None), 1, work_bytes=0)[0] \
        == _lib.DKG_ERR_WORKSPACE  # no discretisation: its pointers may be NULL
    assert run(fake_jobs(1), 1, work=None) == (_lib.DKG_ERR_ARG, "work is NULL")
    jobs = fake_jobs(1)
    jobs[0].o = None
    assert run(jobs, 1) == (_lib.DKG_ERR_ARG, "job 0: o is NULL")
    assert run(fake_jobs(1, N=-1), 1) == (_lib.DKG_ERR_ARG, "job 0: N=-1 discretisation points")
    assert run(fake_jobs(1, jitter=-1.0), 1) == (_lib.DKG_ERR_ARG, "job 0: jitter=-1")
    assert run(fake_jobs(1), 1, d=17) == (_lib.DKG_ERR_UNSUPPORTED, "d=17 (supported 1..16)")


def test_short_workspace():
    lib = _lib.load()
    jobs = fake_jobs(2)
    need = lib.dkg_append_rows_workspace(jobs, 2, 2)
    assert need > 0
    assert run(jobs, 2, work_bytes=need - 1) == (_lib.DKG_ERR_WORKSPACE,
                                                 f"workspace {need - 1} bytes < required {need}")


def test_workspace_size():
    lib = _lib.load()
    ws = lambda **kw: lib.dkg_append_rows_workspace(fake_jobs(**kw), kw.get("J", 1), 2)  # noqa: E731
    base = ws(J=2, n=64, K=3, N=16)
    assert base > 0
    assert ws(J=3, n=64, K=3, N=16) > base and ws(J=2, n=200, K=3, N=16) > base
    assert ws(J=2, n=64, K=3, N=1024) > base and ws(J=2, n=64, K=17, N=16) > base
    assert ws(J=2, n=64, K=3, N=0) > 0
    assert lib.dkg_append_rows_workspace(None, 1, 2) == 0
    assert lib.dkg_append_rows_workspace(fake_jobs(1), 0, 2) == 0
    assert lib.dkg_append_rows_workspace(fake_jobs(513), 513, 2) == 0
    assert lib.dkg_append_rows_workspace(fake_jobs(1), 1, 0) == 0
    for bad in (dict(K=0), dict(K=33), dict(n=1000, K=32), dict(n=0), dict(N=-1)):
        assert ws(**bad) == 0, bad


# --------------------------------------------------------------------------------------------------
# the restatement of the update against LAPACK on the augmented matrix

FAMILIES = [("matern", 0.5), ("matern", 1.5), ("matern", 2.5), ("rbf", 2.5)]


def data(n, kernel, nu, d=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.double)
    y = torch.randn(n, generator=g, dtype=torch.double)
    return SingleTaskGPState(X, y, [0.3, 0.5, 0.9], 2.0, 1e-2, -0.4, kernel, nu)


@pytest.mark.parametrize("kernel,nu", FAMILIES)
@pytest.mark.parametrize("K", [1, 2, 17, 32])
@pytest.mark.parametrize("n", [1, 15, 100])
def test_restatement_matches_cholesky_of_the_augmented_matrix(n, K, kernel, nu):
    """rtol 1e-10 on L' and M', 1e-8 on alpha': test_factor_state_after_chain's tolerances."""
    full = data(n + K, kernel, nu, seed=n + K)
    old = SingleTaskGPState(full.train_x[:n], full.train_y[:n] + 0.5, full.lengthscale, full.outputscale, full.noise,
                            full.mean_constant, full.kernel, full.nu)  # the old targets change with the update
    eye = lambda k: torch.eye(k, dtype=torch.double)  # noqa: E731
    L = torch.linalg.cholesky(covar(old, old.train_x, old.train_x) + old.noise * eye(n))
    M = torch.linalg.solve_triangular(L, eye(n), upper=False)
    D = torch.rand(20, 3, generator=torch.Generator().manual_seed(7), dtype=torch.double)
    QD = covar(old, D, old.train_x) @ M.T
    got = block_update(old, L, M, full.train_x[n:], full.train_y, D=D, QD=QD)
    st = grown(old, full.train_x[n:], full.train_y)
    Kn = covar(st, st.train_x, st.train_x) + st.noise * eye(n + K)
    L_ref = torch.linalg.cholesky(Kn)
    M_ref = torch.linalg.solve_triangular(L_ref, eye(n + K), upper=False)
    r = st.train_y - st.mean_constant
    a_ref = torch.cholesky_solve(r.unsqueeze(-1), L_ref).squeeze(-1)
    torch.testing.assert_close(got["L"], L_ref, rtol=1e-10, atol=1e-11 * L_ref.abs().max().item())
    torch.testing.assert_close(got["M"], M_ref, rtol=1e-10, atol=1e-11 * M_ref.abs().max().item())
    torch.testing.assert_close(got["alpha"], a_ref, rtol=1e-8, atol=1e-9 * a_ref.abs().max().item())
    KD = covar(st, D, st.train_x)
    Q_ref = KD @ M_ref.T
    torch.testing.assert_close(got["QD"], Q_ref, rtol=1e-8, atol=1e-9 * Q_ref.abs().max().item())
    torch.testing.assert_close(got["muD"], st.mean_constant + KD @ a_ref, rtol=1e-8,
                               atol=1e-9 * a_ref.abs().max().item())


def test_restatement_reports_a_covariance_that_is_not_positive_definite():
    X = torch.rand(8, 2, generator=torch.Generator().manual_seed(9), dtype=torch.double)
    y = torch.randn(10, generator=torch.Generator().manual_seed(10), dtype=torch.double)
    old = SingleTaskGPState(X, y[:8], 0.5, 1.0, -1e-9, 0.0)
    L = torch.linalg.cholesky(covar(old, X, X) + old.noise * torch.eye(8, dtype=torch.double))
    M = torch.linalg.solve_triangular(L, torch.eye(8, dtype=torch.double), upper=False)
    X2 = torch.cat([torch.rand(1, 2, generator=torch.Generator().manual_seed(2), dtype=torch.double), X[:1]])
    assert block_update(old, L, M, X2, y) is None
