"""The dominated-space box decomposition of ``include/dkg.h`` on the CPU: the restatement (``boxes_ref.py``) is a
valid partition with the stated volume and count bounds, equals the host function at m = 2 bit for bit, and the C
entries refuse bad arguments before any device work."""
import ctypes
import math

import numpy as np
import pytest
import torch

import boxes_ref as br
from dkg_amd import _lib, metrics
from dkg_amd.jes import compute_sample_box_decomposition

SIZES = (1, 2, 3, 5, 14)
CASES = [(kind, K, m) for m in (2, 3) for K in SIZES for kind in br.KINDS]


@pytest.mark.parametrize("kind,K,m", CASES)
def test_restatement_is_a_partition_with_the_volume_and_the_count_bound(kind, K, m):
    Y, ref = br.case(kind, K, m)
    lo, hi = br.boxes(Y, ref)
    cells, wrong = br.partition_defects(Y, ref, lo, hi)
    assert cells > 0 and wrong == 0
    assert (lo < hi).all()  # no box without an interior
    assert lo.shape[0] <= br.count_bound(K, m)
    # every corner is a copy of an input value or of ref
    values = set(Y.reshape(-1).tolist()) | set(ref.tolist())
    assert set(lo.reshape(-1).tolist()) <= values and set(hi.reshape(-1).tolist()) <= values
    q = br.qualifying(Y, ref)
    ideal = Y[q].max(0) if q else ref
    tol = 8 * br.EPS * float(np.prod(ideal - ref))
    assert abs(float(br.volume_exact(lo, hi)) - metrics.hypervolume(Y, ref)) <= tol


def test_one_objective_is_one_box():
    Y = np.array([[0.5], [2.0], [-3.0], [2.0]])
    lo, hi = br.boxes(Y, np.array([-1.0]))
    assert lo.tolist() == [[-1.0]] and hi.tolist() == [[2.0]]
    lo, hi = br.boxes(Y, np.array([2.0]))
    assert lo.shape == (0, 1)


@pytest.mark.parametrize("maximize", [True, False])
def test_two_objective_restatement_equals_the_host_function(maximize):
    ref = np.full(2, -1e10)
    fronts = [br.case(kind, K, 2, seed=1)[0] for kind, K in (("cloud", 14), ("front", 5), ("lattice", 14),
                                                             ("equal", 3), ("cloud", 1))]
    want = compute_sample_box_decomposition([torch.from_numpy(f if maximize else -f) for f in fronts],
                                            maximize=maximize)
    got, count = br.padded(fronts, ref)
    if not maximize:
        mirrored = np.zeros_like(got)
        for s, c in enumerate(count):
            mirrored[s, 0, :c], mirrored[s, 1, :c] = -got[s, 1, :c], -got[s, 0, :c]
        got = mirrored
    assert got.shape == tuple(want.shape)
    assert got.tobytes() == want.numpy().tobytes()


@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_lattice_antichain_volume_is_a_binomial(n):
    Y, ref = br.antichain(n)
    lo, hi = br.boxes(Y, ref)
    assert lo.shape[0] == Y.shape[0]  # one box per point
    assert br.volume_exact(lo, hi) == math.comb(n + 2, 3)
    assert br.partition_defects(Y, ref, lo, hi)[1] == 0


def test_slab_partition_is_a_partition_too():
    Y, ref = br.case("cloud", 14, 3)
    lo, hi = br.slab_boxes(Y, ref)
    assert br.partition_defects(Y, ref, lo, hi)[1] == 0
    assert lo.shape[0] > br.boxes(Y, ref)[0].shape[0]


def test_c_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    ref = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    E_ARG, E_UNS, E_WS = _lib.DKG_ERR_ARG, _lib.DKG_ERR_UNSUPPORTED, _lib.DKG_ERR_WORKSPACE
    big = 1 << 40

    def boxes(Y=16, S=1, K=4, m=3, r=ref, J=7, bounds=16, count=16, work=16, nbytes=big):
        return lib.dkg_dominated_boxes(Y, S, K, m, r, J, bounds, count, work, nbytes, None)

    def hv(Y=16, S=1, K=4, m=3, r=ref, out=16, work=16, nbytes=big):
        return lib.dkg_hypervolume_front(Y, S, K, m, r, out, work, nbytes, None)

    # NULL pointers
    for kw in ({"Y": None}, {"r": None}, {"bounds": None}, {"count": None}, {"work": None}):
        assert boxes(**kw) == E_ARG, kw
    for kw in ({"Y": None}, {"r": None}, {"out": None}, {"work": None}):
        assert hv(**kw) == E_ARG, kw
    # sizes < 1
    for kw in ({"S": 0}, {"K": 0}, {"m": 0}):
        assert boxes(**kw) == E_ARG and hv(**kw) == E_ARG, kw
    # J below the count bound: 1 / K / 2K - 1
    assert boxes(m=1, J=0) == E_ARG
    assert boxes(m=2, J=3) == E_ARG
    assert boxes(m=3, J=6) == E_ARG and b"J=6" in lib.dkg_last_error()
    # beyond the limits
    assert boxes(m=4, J=64) == E_UNS and hv(m=4) == E_UNS
    assert boxes(K=_lib.DKG_BOXES_MAX_POINTS + 1, J=4096) == E_UNS
    assert boxes(K=8, m=3, J=_lib.DKG_JES_MAX_BOXES + 1) == E_UNS
    assert hv(K=_lib.DKG_HV_FRONT_MAX_POINTS + 1) == E_UNS
    # a short workspace
    need_b = lib.dkg_dominated_boxes_workspace(2, 2048, 3)
    need_h = lib.dkg_hypervolume_front_workspace(2, 16384, 3)
    assert need_b >= 2 * 2048 * 40 and need_h >= 2 * 16384 * 40
    assert boxes(S=2, K=2048, J=4095, nbytes=need_b - 1) == E_WS
    assert hv(S=2, K=16384, nbytes=need_h - 1) == E_WS
    # the workspace sizes of refused shapes are 0
    assert lib.dkg_dominated_boxes_workspace(1, 2049, 3) == 0 and lib.dkg_dominated_boxes_workspace(1, 4, 4) == 0
    assert lib.dkg_hypervolume_front_workspace(1, 16385, 3) == 0 and lib.dkg_hypervolume_front_workspace(0, 4, 3) == 0
    assert lib.dkg_hypervolume_front_workspace(1, 16384, 3) > 0
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(hv(m=4), "dkg_hypervolume_front")


def test_jes_spec_points_three_objectives_to_the_device_boxes():
    """``compute_sample_box_decomposition`` still raises at m = 3 and names the device function."""
    from dkg_amd import dominated_boxes, hypervolume_front  # noqa: F401  exported
    from dkg_amd.errors import UnsupportedError

    with pytest.raises(UnsupportedError):
        compute_sample_box_decomposition([torch.rand(4, 3)])
    assert "dominated_boxes" in compute_sample_box_decomposition.__doc__
