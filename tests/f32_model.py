"""The rounding model of the fp32 plan's two contractions (DKG_PLAN_F32: Q_X = K(x, X) R and Q_X Q_D^T on
v_mfma_f32_16x16x4_f32), the reference both test_f32_model_host.py (CPU) and test_gpu_f32_model.py (device) hold
the kernels to, and the matrix of shapes they run.  torch fp64 on the CPU throughout.

The model.  Each stage is one contraction c = sum_i a_i b_i of fp32 operands a_i, b_i.  Given the operands
exactly, a result computed in fp32 (round to nearest, u = 2^-24) differs from the exact sum of the exact products
by accumulation rounding alone.  With one rounding per product and one per addition, a product passes through
at most one product rounding and, whatever the order of the additions (a chain, chains per wave, the MFMA's
4-wide blocks, interleaved accumulators, partial sums met in fp64), through at most n_pad - 1 additions, n_pad
the padded length of the contraction (the zero padding takes part in the additions).  So (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 3.1: the bound holds for any summation order)

    |c_fp32 - c| <= gamma_(n_pad) sum_i |a_i| |b_i|,   gamma_k = k u / (1 - k u).

The constant C0 = 4 adds to n_pad:

  1  the store: the cross stage rounds its result once more to fp32 (Plan::q32).  (The covariance stage stores
     kappa - sum in fp64: it has no such rounding and keeps the unit as slack.)
  1  everything of second order and everything fp64: gamma_k against k u (k u <= 1024 * 2^-24 = 6.1e-5, so
     gamma_k <= k u (1 + 6.2e-5), far below one u in (k + 1) u), and the fp64 roundings where partial sums meet
     (2^-53 each).
  2  one operand taken from the oracle instead of the device.  The oracle's fp64 value may differ from the
     device's in its last places; its fp32 rounding then differs only where the value sits within that distance
     of a rounding tie, and there by one fp32 ulp, which is at most 2 u relative to the value (an ulp is 2^-23
     of the binade's lower end).  The cross stage takes K(x, X) from the oracle (the device evaluates it inside
     the kernel and keeps no copy) and R from the device (OutputCache.Linv, row-major); the covariance stage
     takes Q_D from the oracle (the device holds it fragment-packed only) and Q_X from the device (the exported
     fp32 Q_X, exact).  One oracle operand per stage: 2.  (The CPU tests take both operands from the oracle and
     compare emulations on those same operands, so there the 2 is slack.)

C0 is derived, not fitted: a device result outside the bound is a finding.

Per stage, not end to end: the cross stage's bound carried through the covariance stage is multiplied by Q_D's
entries and exceeds the covariance itself at n >= 512, so the covariance reference starts from the device's own
exported Q_X32.  What the cross stage got wrong is the cross check's to find.
"""

import math

import torch

from helpers import ALL_FAMILIES, LINE_RTOL, grad_case, to_oracle
from oracle.discretekg import coincident_index

U = 2.0 ** -24
C0 = 4


def pad16(x: int) -> int:
    return (x + 15) & ~15


def fl32(t: torch.Tensor) -> torch.Tensor:
    """t rounded to fp32 (round to nearest even), as fp64."""
    return t.to(torch.float32).to(torch.double)


def bound(n_pad: int, absA: torch.Tensor, absB: torch.Tensor) -> torch.Tensor:
    """(n_pad + C0) u |A| |B|."""
    return (n_pad + C0) * U * (absA @ absB)


# ---------------------------------------------------------------------------------------------- the matrix
# T = n_pad / 16 column tiles of Q_X per output (cross_root_impl pairs tile p with tile T - 1 - p: an odd T
# pairs the middle tile with itself).  Cross stage: cross_big32_kernel iff cross_kfill_launch(max n_pad, B):
# max n_pad >= 512 or B >= 512 (csrc/dkg_kernels.h), else cross_root_plan_kernel<DM, float> with
# grid (pad16(B) / 16, groups, m).  Covariance stage: posterior_cov_big32_kernel<DM> iff DM <= 8, N >= 128 and
# ceil(N / 64) ceil(B / 64) m >= 256 (cov_big, csrc/dkg_kernels.hip), its 64 x 64 blocks in order 1 iff
# nbx >= 4 nby; else posterior_cov_kernel<DM, float>'s 32 x 32 blocks.  `cov_blocks` = (nbx, nby, order) as the
# dispatch query returns them (order -1: the narrow kernel).
def _case(id, m, d, ns, N, B, cross, cov, cov_blocks, what, coincide=None, **kw):
    return dict(id=id, m=m, d=d, ns=tuple(ns), N=N, B=B, cross=cross, cov=cov, cov_blocks=cov_blocks, what=what,
                coincide=coincide, kw=kw)


MATRIX = [
    _case("n-min", 1, 1, (1,), 1, 1, "narrow", "narrow", (1, 1, -1), "every extent 1; T = 1"),
    _case("n-odd", 2, 3, (37, 17), 100, 17, "narrow", "narrow", (4, 1, -1),
          "T = 3 (middle tile pairs with itself) and T = 2; candidate 3 placed on row 7 of D", coincide=(3, 7)),
    _case("n-mixed", 3, 6, (16, 48, 200), 33, 33, "narrow", "narrow", (2, 2, -1),
          "T = 1, 3, 13; n_pad 208; narrow outputs under a wide max_np"),
    _case("n-d16", 2, 11, (100, 64), 150, 5, "narrow", "narrow", (5, 1, -1), "DM = 16; T = 7, 4"),
    _case("n-m5", 5, 2, (40, 33, 20, 64, 15), 31, 16, "narrow", "narrow", (1, 1, -1),
          "padded output bucket (m = 5 in the bucket of 8); T = 3, 3, 2, 4, 1"),
    _case("n-496", 1, 2, (496,), 64, 3, "narrow", "narrow", (2, 1, -1), "largest n_pad below the fill rule; T = 31"),
    _case("x-np", 2, 2, (497, 40), 100, 5, "big32", "narrow", (4, 1, -1),
          "fill by n_pad = 512 (T = 32), with a far narrower second output (T = 3); lengthscale 0.1: at the "
          "default one the last column of Q_X (one live column in tile 31) is smaller than its own bound, and a "
          "stale last tile was flagged by 0.45 of it only", lengthscale=0.1),
    _case("x-rag", 1, 4, (530,), 40, 70, "big32", "narrow", (2, 3, -1),
          "n_pad 544 (T = 34, 17 column blocks of 2 tiles); B = 70: 5 row tiles, the second row block 1 tile"),
    _case("x-B", 3, 8, (20, 33, 16), 20, 520, "big32", "narrow", (1, 17, -1),
          "fill by B >= 512 with tiny n (T = 2, 3, 1); 33 row tiles, 9 row blocks of 4, the last 1 tile"),
    _case("x-d16", 1, 11, (512,), 130, 4, "big32", "narrow", (5, 1, -1),
          "the fill's DM = 16; the covariance stage excluded from big32 (d > 8)"),
    _case("c-edge", 8, 2, (20,), 2000, 20, "narrow", "big32", (32, 1, 1),
          "exactly 256 blocks (32 x 1 x 8); last column block 16 wide; one partial row block"),
    _case("c-below", 8, 2, (20,), 1984, 20, "narrow", "narrow", (62, 1, -1),
          "31 x 1 x 8 = 248 blocks of 64 x 64: the other side of the threshold"),
    _case("c-ord1", 3, 5, (40, 100, 17), 4100, 70, "narrow", "big32", (65, 2, 1),
          "65 x 2 blocks, the last 4 lines wide, the second row block 6 rows; block order 1"),
    _case("c-ord0", 8, 8, (20,), 1100, 300, "narrow", "big32", (18, 5, 0), "18 x 5 blocks, block order 0"),
    _case("c-d16", 8, 11, (20,), 2000, 20, "narrow", "narrow", (63, 1, -1), "DM = 16 keeps the narrow kernel"),
    _case("xc", 4, 3, (530,), 2053, 70, "big32", "big32", (33, 2, 1), "both block kernels in one forward"),
]
ROWS = {r["id"]: r for r in MATRIX}
S = 2


def targets_of(row):
    """None, output 0 and the last output (once each)."""
    return [None, 0] + ([row["m"] - 1] if row["m"] > 1 else [])


def max_np_of(row) -> int:
    return max(pad16(row["ns"][i % len(row["ns"])]) for i in range(row["m"]))


def problem(row):
    """The row's problem from helpers.grad_case (S = 2, the families cycling over ALL_FAMILIES, default noise
    unless the row's ``kw`` says otherwise): (state, D, W, X)."""
    seed = 100 + [r["id"] for r in MATRIX].index(row["id"])
    state, D, W, X = grad_case(row["m"], row["d"], row["ns"], ALL_FAMILIES, row["N"], S, row["B"], seed, **row["kw"])
    if row["coincide"] is not None:
        b, k = row["coincide"]
        X = X.clone()
        X[b] = D[k]
    return state, D, W, X


# ---------------------------------------------------------------------------------------------- operands
def operands(om, X, D, Linv=None):
    """The fp32 operands of one output (oracle OutputGP ``om``), as fp64 tensors: K32 = fl32(K(x, X)) [B, n],
    R32 = fl32(R) [n, n] (R = L^-T: from the device's row-major L^-1 ``Linv`` when given, else the oracle's),
    QD32 = fl32(Q_D) [N, n] with Q_D = K(D, X) R, and the fp64 kernel block K(x, D) [B, N]."""
    n = om.train_x.shape[0]
    c = om.cache()
    Kx = om.covar(X, torch.cat([om.train_x, X], 0))[:, :n]  # (the rows oracle.lines_batched evaluates)
    Kd = om.covar(D, torch.cat([om.train_x, D], 0))[:, :n]
    R = c["R"] if Linv is None else Linv.detach().cpu().double().mT
    return {"K32": fl32(Kx), "R32": fl32(R), "QD32": fl32(Kd @ c["R"]), "kxd": om.covar(X, D)}


def cross_reference(op):
    """Q_X of the exact operands, and its bound E1 [B, n]."""
    n_pad = pad16(op["K32"].shape[1])
    return op["K32"] @ op["R32"], bound(n_pad, op["K32"].abs(), op["R32"].abs())


def cov_reference(om, op, QX32):
    """From the fp32 Q_X the covariance stage read (``QX32`` [B, n], fp64 values of fp32 numbers): the variance
    v = s - sum Q_X32^2 [B] (fp64, as the kernels form it), the covariance rows s kappa(x, D_k) - Q_X32 . QD32_k
    [B, N], and their bound E2 [B, N]."""
    n_pad = pad16(QX32.shape[1])
    v = om.outputscale - (QX32 * QX32).sum(-1)
    cov = op["kxd"] - QX32 @ op["QD32"].mT
    return v, cov, bound(n_pad, QX32.abs(), op["QD32"].abs().mT)


def slopes_reference(model, X, D, W, target, vs, covs, E2s):
    """The slopes oracle.lines_batched builds, from per-output v [B], cov [B, N] and the covariance bound E2
    [B, N]: b [B, S, N + 1] and its tolerance.  The slopes are linear in cov once v is fixed, so the tolerance is
    E2 through the same linear map; line 0 of a candidate that sits on no discretisation point carries only v
    (fp64 sums of the same fp32 numbers), and takes the fp64 floor alone: LINE_RTOL max |b|, the agreement the
    project requires of two fp64 builds of the lines (helpers.LINE_RTOL).  A candidate on discretisation point k
    has line 0 a copy of line k + 1 (oracle.discretekg.coincident_index), bound included."""
    B = X.shape[0]
    cv, ev, vn = [], [], []
    for om, v, cov, E2 in zip(model.models, vs, covs, E2s):
        sd2 = om.y_std ** 2
        cv.append(torch.cat([v[:, None], cov], 1) * sd2)
        ev.append(torch.cat([torch.zeros(B, 1, dtype=torch.double), E2], 1) * sd2)
        vn.append((v + om.noise) * sd2)
    cv, ev, vn = torch.stack(cv, -1), torch.stack(ev, -1), torch.stack(vn, -1)  # [B, N + 1, m] x 2, [B, m]
    for bi in range(B):
        kc = coincident_index(X[bi], D)
        if kc is not None:
            cv[bi, 0] = cv[bi, kc + 1]
            ev[bi, 0] = ev[bi, kc + 1]
    if target is None:
        den = torch.einsum("bm,sm->bs", vn, W ** 2).sqrt()[..., None]
        b = torch.einsum("bkm,sm->bsk", cv, W ** 2) / den
        tol = torch.einsum("bkm,sm->bsk", ev, W ** 2) / den
    else:
        den = vn[:, target].sqrt()[:, None, None]
        b = W[None, :, target, None] * cv[:, None, :, target] / den
        tol = W[None, :, target, None].abs() * ev[:, None, :, target] / den
    return b, tol + LINE_RTOL * b.abs().max()


# ---------------------------------------------------------------------------------------------- emulations
def emulate(A, Bm, order):
    """A @ Bm summed in fp32 (every product and every partial sum rounded to fp32) in one of the orders
    "seq" (k ascending), "rev" (k descending), "c4" / "c64" (chunks of 4 / 64 summed ascending from zero, then
    the chunk sums ascending).  A [M, K], Bm [K, N]: fp64 tensors holding fp32 values.  -> fp64 [M, N]."""
    A32, B32 = A.to(torch.float32), Bm.to(torch.float32)
    M, K = A32.shape
    N = B32.shape[1]
    zero = lambda: torch.zeros(M, N, dtype=torch.float32)  # noqa: E731
    prod = lambda k: A32[:, k, None] * B32[None, k, :]  # noqa: E731

    def chain(ks):
        acc = zero()
        for k in ks:
            acc = acc + prod(k)
        return acc

    if order == "seq":
        out = chain(range(K))
    elif order == "rev":
        out = chain(range(K - 1, -1, -1))
    else:
        c = {"c4": 4, "c64": 64}[order]
        out = zero()
        for k0 in range(0, K, c):
            out = out + chain(range(k0, min(K, k0 + c)))
    return out.to(torch.double)


EMULATIONS = ("seq", "rev", "c4", "c64")


# ---------------------------------------------------------------------------------------------- mutations
def frag32_index(t, kb, l, KB):
    """csrc/dkg_common.h frag32_index: element (16 t + (l & 15), 4 kb + (l >> 4)) of a quad-packed matrix."""
    return ((t * (KB >> 2) + (kb >> 2)) * 64 + l) * 4 + (kb & 3)


def _padded(A, Bm):
    M, K = A.shape
    N = Bm.shape[1]
    Ap = torch.zeros(pad16(M), pad16(K), dtype=torch.double)
    Bp = torch.zeros(pad16(K), pad16(N), dtype=torch.double)
    Ap[:M, :K] = A
    Bp[:K, :N] = Bm
    return Ap, Bp


# D row 4 a + r of the f32 map written where the f64 map puts (a, r): row a + 4 r
_F64_FOR_F32 = torch.tensor([(i >> 2) + 4 * (i & 3) for i in range(16)])


def mutate(A, Bm, kind, d_rows_are_columns=False):
    """The contraction A @ Bm (exact, fp64, of fp32 operands) with one structured mistake, or None where the
    shape has no place for it.  Tiles are 16 x 16, k-blocks 4 wide, over the zero-padded operands; the result
    is cut back to [M, N].

      drop     one k-block (k-block 0) left out of the last column tile of row tile 0
      swap     k-blocks 0 and 1 (one quad) of A exchanged, B's left in place, same tile
      tiles    column tiles 0 and 1 exchanged (needs two column tiles)
      stale    the last partial row tile computed with the previous row tile's A rows, else the last partial
               column tile with the previous column tile's B columns (needs such a tile and one before it)
      dmap     tile (0, 0) written by the f64 D map (row (l >> 4) + 4 r) in place of the f32 one
               (row 4 (l >> 4) + r): the D rows are the output's rows (covariance stage) or its columns (cross
               stage, D = R^T K^T: ``d_rows_are_columns``); needs a live D row that moves
    """
    M, N = A.shape[0], Bm.shape[1]
    Ap, Bp = _padded(A, Bm)
    C = Ap @ Bp
    Tr, Tc = C.shape[0] // 16, C.shape[1] // 16
    rows, cols = slice(0, 16), slice(16 * (Tc - 1), 16 * Tc)
    if kind == "drop":
        C[rows, cols] -= Ap[rows, 0:4] @ Bp[0:4, cols]
    elif kind == "swap":
        C[rows, cols] += (Ap[rows, 4:8] - Ap[rows, 0:4]) @ Bp[0:4, cols] + (Ap[rows, 0:4] - Ap[rows, 4:8]) @ Bp[4:8, cols]
    elif kind == "tiles":
        if Tc < 2:
            return None
        C[:, 0:32] = torch.cat([C[:, 16:32], C[:, 0:16]], 1)
    elif kind == "stale":
        if M % 16 and Tr >= 2:
            C[16 * (Tr - 1):] = Ap[16 * (Tr - 2):16 * (Tr - 1)] @ Bp
        elif N % 16 and Tc >= 2:
            C[:, 16 * (Tc - 1):] = Ap @ Bp[:, 16 * (Tc - 2):16 * (Tc - 1)]
        else:
            return None
    elif kind == "dmap":
        live = N if d_rows_are_columns else M
        if all(int(_F64_FOR_F32[i]) == i for i in range(min(live, 16))):
            return None
        t = C[0:16, 0:16].clone()
        if d_rows_are_columns:
            C[0:16, _F64_FOR_F32] = t
        else:
            C[_F64_FOR_F32, 0:16] = t
    else:
        raise ValueError(kind)
    return C[:M, :N]


def mutate_stride(Q, max_np):
    """A narrow output's Q_X [B, n] stored quad-packed with its own n_pad and read back with the widest
    output's (KB = max_np / 4): words past the buffer read as zero.  None when the output is the widest, or
    when there is one row tile (tile 0 starts at 0 whatever KB is: the mistake changes nothing there)."""
    B, n = Q.shape
    np_, Bp = pad16(n), pad16(B)
    if np_ >= max_np or Bp == 16:
        return None
    r = torch.arange(Bp)[:, None].expand(Bp, np_)
    c = torch.arange(np_)[None, :].expand(Bp, np_)
    lane = ((c & 3) << 4) | (r & 15)
    Qp = torch.zeros(Bp, np_, dtype=torch.double)
    Qp[:B, :n] = Q
    packed = torch.zeros(Bp * np_, dtype=torch.double)
    packed[frag32_index(r >> 4, c >> 2, lane, np_ // 4).reshape(-1)] = Qp.reshape(-1)
    wide = frag32_index(r >> 4, c >> 2, lane, max_np // 4).reshape(-1)
    ok = wide < packed.numel()
    out = torch.zeros(Bp * np_, dtype=torch.double)
    out[ok] = packed[wide[ok]]
    return out.reshape(Bp, np_)[:B, :n]


MUTATIONS = ("drop", "swap", "tiles", "stale", "dmap")


def worst_ratio(got, ref, E, floor=0.0):
    """max |got - ref| / (E + floor) (0 / 0 counts as 0)."""
    err = (got - ref).abs()
    tol = E + floor
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(ratio.max()) if ratio.numel() else 0.0


def oracle_model(state):
    return to_oracle(state)
