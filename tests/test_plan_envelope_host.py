"""The host side of dkg_debug_plan_envelope (include/dkg.h): which envelope kernel a plan launches, read from
the host plan.  It touches no device, so its argument handling needs no GPU; what it reports for real plans is
asserted case by case in tests/test_gpu_grad_matrix.py."""

import ctypes

from dkg_amd import _lib


def test_null_pointers_are_refused_and_nothing_is_written():
    lib = _lib.load()
    out = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert lib.dkg_debug_plan_envelope(None, out) == -2
    assert b"dkg_debug_plan_envelope" in lib.dkg_last_error()
    assert list(out) == [7, 7, 7, 7]
    blank = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    assert lib.dkg_debug_plan_envelope(blank, None) == -2
    assert lib.dkg_debug_plan_envelope(None, None) == -2


def test_a_plan_never_initialised_reads_as_the_empty_staged_plan():
    """All-zero plan bytes: N = 0 (one line, the 2-slot kernel), not streaming, no geometry yet."""
    lib = _lib.load()
    blank = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    out = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert lib.dkg_debug_plan_envelope(blank, out) == 0
    assert list(out) == [2, 0, 0, 0]


def test_the_call_changes_nothing_in_the_plan():
    lib = _lib.load()
    n = lib.dkg_plan_bytes()
    blank = ctypes.create_string_buffer(n)
    out = (ctypes.c_int * 4)()
    assert lib.dkg_debug_plan_envelope(blank, out) == 0
    assert blank.raw == bytes(n)
