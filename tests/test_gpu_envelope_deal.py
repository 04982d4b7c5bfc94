"""The envelope launches deal their candidates over the XCDs by xcd_deal (csrc/dkg_common.h), not in index order.
Which workgroup runs an item changes no arithmetic, so a launch over B candidates must write, bit for bit, what
the same plan writes in one call per candidate (a launch of one item, where the map is the identity): KG, KG per
pair, the envelope sizes and dKG/dx.  The shapes are those where a wrong map shows: a ragged last group of eight
items (B = 1, 7, 9, 63, 65, 130), the padding ids, q / 8 > 0 (B > 64), and one, two and three workgroups per
item (S = 8, 16, 24); plans of two targets, the gradient kernels, the global-rows gradient kernels and a launch
of three batches.  The problem (m 2, n 48, an 8 x 8 grid, d 2) has pairs the flat test settles and pairs that
are walked.  (The map itself, larger item counts included: tests/test_envelope_deal_host.py.)
"""
import pytest
import torch

from dkg_amd import DiscreteKnowledgeGradient
from dkg_amd.synthetic import Workload, make_problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BMAX = 130
SIZES = (1, 7, 8, 9, 63, 65, 130)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")


class _Case:
    """One problem per S: its plans, the candidates, and the one-call-per-candidate results (computed once)."""

    def __init__(self, S):
        w = Workload("deal", m=2, n_train=48, grid=8, S=S, B=BMAX)
        model, D, X, W = make_problem(w)
        self.acq = DiscreteKnowledgeGradient(model, D, W, device=DEV)
        self.X = X.to(DEV).contiguous()
        self.S = S
        self._plans = {}
        self._ref = {}

    def plan(self, **kw):
        key = tuple(sorted(kw.items(), key=lambda kv: kv[0]))
        if key not in self._plans:
            kw = dict(kw)
            if "targets" in kw:
                kw["targets"] = list(kw["targets"])
            self._plans[key] = self.acq._state.plan(self.acq._W, self.acq._target, BMAX, **kw)
        return self._plans[key]

    def forward(self, plan, X):
        kg = torch.full(plan._lead(X.shape[0]), float("nan"), dtype=torch.double, device=DEV)
        plan.forward_into(X, kg)
        return kg

    def per_candidate(self, what, n, **kw):
        """Rows 0..n-1 of `what` ("forward", "stats", "grad") from one call per candidate on the plan of **kw
        (computed once per plan and kept), joined along the candidate axis."""
        key = (what, tuple(sorted(kw.items(), key=lambda kv: kv[0])))
        have = self._ref.setdefault(key, [])
        plan = self.plan(**kw)
        for b in range(len(have), n):
            x = self.X[b:b + 1]
            if what == "forward":
                have.append((self.forward(plan, x).cpu(),))
            elif what == "stats":
                have.append(tuple(t.cpu() for t in plan.forward_stats(x)))
            else:
                have.append(tuple(t.cpu() for t in plan.forward_grad(x)))
        axis = 0 if plan.targets is None else 1
        return tuple(torch.cat([h[i] for h in have[:n]], dim=axis) for i in range(len(have[0])))


_cases = {}


@pytest.fixture(params=[8, 16, 24], ids=lambda S: f"S{S}")
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    return _cases[request.param]


def _same(got, ref):
    return got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(
        got.view(torch.int64) if got.dtype == torch.double else got, ref.view(torch.int64) if ref.dtype == torch.double else ref)


@pytest.mark.parametrize("B", SIZES)
def test_forward_writes_the_per_candidate_bits(case, B):
    plan = case.plan()
    assert plan.envelope_geometry()["split"] == case.S // 8
    kg = case.forward(plan, case.X[:B]).cpu()
    (ref,) = case.per_candidate("forward", B)
    assert not torch.isnan(ref).any()
    assert _same(kg, ref)
    # the pairs path (every pair walked: it also records the envelope sizes)
    _, pairs, hull = (t.cpu() for t in plan.forward_stats(case.X[:B]))
    rkg, rpairs, rhull = case.per_candidate("stats", B)
    assert _same(pairs, rpairs) and _same(hull, rhull)
    assert _same(rkg, ref)  # the flat test returns the walk's value
    if B >= 63:  # both kinds of pair: settled by the flat test (KG = 0 exactly) and walked
        assert (rpairs == 0).any() and (rpairs > 0).any()


def test_forward_grad_writes_the_per_candidate_bits(case):
    kg, dkg = (t.cpu() for t in case.plan(grad=True).forward_grad(case.X[:9]))
    rkg, rdkg = case.per_candidate("grad", 9, grad=True)
    assert not torch.isnan(rdkg).any() and (rdkg != 0).any()
    assert _same(kg, rkg) and _same(dkg, rdkg)


def test_global_rows_gradient_writes_the_per_candidate_bits(case):
    plan = case.plan(grad=True, grad_rows="global")
    assert plan.grad_rows_global
    kg, dkg = (t.cpu() for t in plan.forward_grad(case.X[:9]))
    rkg, rdkg = case.per_candidate("grad", 9, grad=True, grad_rows="global")
    assert _same(kg, rkg) and _same(dkg, rdkg)


def test_two_targets_write_the_per_candidate_bits(case):
    targets = (None, 1)
    kg, pairs, hull = (t.cpu() for t in case.plan(targets=targets).forward_stats(case.X[:9]))
    rkg, rpairs, rhull = case.per_candidate("stats", 9, targets=targets)
    assert kg.shape == (2, 9) and not torch.isnan(rkg).any()
    assert _same(kg, rkg) and _same(pairs, rpairs) and _same(hull, rhull)
    fkg = case.forward(case.plan(targets=targets), case.X[:9]).cpu()
    (rf,) = case.per_candidate("forward", 9, targets=targets)
    assert _same(fkg, rf)
    gkg, gd = (t.cpu() for t in case.plan(targets=targets, grad=True).forward_grad(case.X[:9]))
    rgkg, rgd = case.per_candidate("grad", 9, targets=targets, grad=True)
    assert _same(gkg, rgkg) and _same(gd, rgd)
    gkg, gd = (t.cpu() for t in case.plan(targets=targets, grad=True, grad_rows="global").forward_grad(case.X[:9]))
    rgkg, rgd = case.per_candidate("grad", 9, targets=targets, grad=True, grad_rows="global")
    assert _same(gkg, rgkg) and _same(gd, rgd)


def test_three_batches_write_the_per_candidate_bits(case):
    plan = case.plan()
    kg = torch.full((27,), float("nan"), dtype=torch.double, device=DEV)
    plan.forward_batches_into(case.X[:27], kg, 9)
    (ref,) = case.per_candidate("forward", 27)
    assert _same(kg.cpu(), ref)
