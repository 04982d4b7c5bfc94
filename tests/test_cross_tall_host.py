"""The host side of the one-launch cross kernel's dispatch (include/dkg.h dkg_debug_cross_tall,
dkg_debug_cross_tall_eligible): the mode switch's argument handling and the eligibility rule.  Both are
host code that touches no device, so they need no GPU."""

import pytest

from dkg_amd import _lib


@pytest.fixture
def lib():
    lib = _lib.load()
    prev = lib.dkg_debug_cross_tall(-1)
    yield lib
    lib.dkg_debug_cross_tall(prev)


def test_mode_switch_returns_the_previous_mode(lib):
    assert lib.dkg_debug_cross_tall(0) == -1
    assert lib.dkg_debug_cross_tall(1) == 0
    assert lib.dkg_debug_cross_tall(-1) == 1
    assert lib.dkg_debug_cross_tall(-1) == -1


@pytest.mark.parametrize("bad", [-3, -2, 2, 7, 1 << 20])
def test_mode_switch_rejects_other_values(lib, bad):
    lib.dkg_debug_cross_tall(1)
    assert lib.dkg_debug_cross_tall(bad) == -2
    assert b"dkg_debug_cross_tall" in lib.dkg_last_error()
    assert lib.dkg_debug_cross_tall(-1) == 1  # the rejected call changed nothing


def test_default_rule_is_the_candidate_count(lib):
    el = lib.dkg_debug_cross_tall_eligible
    assert el(256, 2, 512, 0) == 1 and el(256, 2, 640, 0) == 1 and el(256, 2, 2560, 0) == 1
    assert el(256, 2, 511, 0) == 0 and el(256, 2, 128, 0) == 0 and el(256, 2, 1, 0) == 0
    assert el(16, 1, 512, 0) == 1 and el(112, 6, 600, 0) == 1 and el(256, 16, 512, 0) == 1


def test_wide_outputs_and_fp32_plans_never_take_it(lib):
    el = lib.dkg_debug_cross_tall_eligible
    for mode in (-1, 1):
        lib.dkg_debug_cross_tall(mode)
        assert el(272, 2, 640, 0) == 0   # more column-tile pairs than waves
        assert el(512, 2, 640, 0) == 0 and el(1024, 2, 512, 0) == 0  # the stress shape
        assert el(256, 2, 640, 1) == 0 and el(64, 2, 640, 1) == 0    # DKG_PLAN_F32


def test_forced_modes(lib):
    el = lib.dkg_debug_cross_tall_eligible
    lib.dkg_debug_cross_tall(1)
    assert el(256, 2, 1, 0) == 1 and el(16, 1, 15, 0) == 1 and el(112, 6, 130, 0) == 1 and el(256, 2, 640, 0) == 1
    lib.dkg_debug_cross_tall(0)
    assert el(256, 2, 640, 0) == 0 and el(256, 2, 1, 0) == 0 and el(16, 1, 4096, 0) == 0


@pytest.mark.parametrize("args", [(0, 2, 640, 0), (250, 2, 640, 0), (-16, 2, 640, 0), (256, 0, 640, 0),
                                  (256, 17, 640, 0), (256, 2, 0, 0), (256, 2, -5, 0)])
def test_eligibility_rejects_bad_arguments(lib, args):
    assert lib.dkg_debug_cross_tall_eligible(*args) == -2
    assert b"dkg_debug_cross_tall_eligible" in lib.dkg_last_error()


def test_launch_counter_is_readable_without_a_device(lib):
    assert lib.dkg_debug_cross_tall_launches() >= 0
