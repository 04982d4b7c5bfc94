"""Where the staged forward envelope hands its pair coefficients over (csrc/dkg_device.h envelope_body, COEF1),
checked on the host against the kernels' own layout (dkg_debug_envelope_lds).  CPU only.

Wave 0 writes pair p's row (wa[M] | wb[M] | a_off | line 0's a, b: 2 M + 3 doubles) at the head of wave p's
survivor list, sbuf + p * 2 * LC, before the staging barrier; wave p reads it after the barrier and only then
writes its list.  The change adds no LDS region and no static LDS, so this file pins what it relies on: every row
lies inside the sbuf region of the forward-staged layout, rows of different waves do not overlap, and the
layout's total is still the one tests/envelope_lds_ref.py transcribes (what decides how many workgroups fit a CU).
"""

import ctypes
import itertools

import pytest

import envelope_lds_ref as ref
from dkg_amd import _lib

NREG = 20
SBUF, CBUF, SIF = 5, 6, 7          # region indices (tests/test_envelope_lds_host.py REGIONS)
LC = 128                           # survivor-list capacity per wave of the staged kernels (ENV_CAP)
FORWARD_STAGED = (0, 0, 0)


def layout(m, N, waves, S):
    out = (ctypes.c_int * (NREG + 1))()
    assert _lib.load().dkg_debug_envelope_lds(m, N, waves, S, 2, 256, *FORWARD_STAGED, out) == _lib.DKG_OK
    return list(out)


@pytest.mark.parametrize("m", range(1, 9))
def test_rows_lie_in_their_waves_lists(m):
    M = ref.outputs_bucket(m)
    row = 2 * M + 3
    assert row <= 2 * LC
    for N, waves in itertools.product((0, 1, 90, 127, 128, 300, 511, 560, 1024, 1087, 2111), (1, 2, 3, 8)):
        for S in {waves, waves + 3, 40}:
            off = layout(m, N, waves, S)
            sbuf, end = off[SBUF], off[CBUF]           # cbuf is empty when the lines are staged: sif starts there
            assert off[CBUF] == off[SIF] and end - sbuf == waves * 2 * LC, (m, N, waves, S)
            rows = [(sbuf + p * 2 * LC, sbuf + p * 2 * LC + row) for p in range(waves)]
            assert rows[0][0] == sbuf and rows[-1][1] <= end
            assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:]))
            # and nothing about the totals moved
            assert off[NREG] * 8 == ref.envelope_lds_bytes(m, N, waves, S, False), (m, N, waves, S)


def test_bad_arguments_are_still_refused():
    lib = _lib.load()
    out = (ctypes.c_int * (NREG + 1))()
    assert lib.dkg_debug_envelope_lds(2, 1024, 9, 16, 2, 256, *FORWARD_STAGED, out) == _lib.DKG_ERR_ARG
    assert lib.dkg_debug_envelope_lds(2, 1024, 8, 16, 2, 256, *FORWARD_STAGED, None) == _lib.DKG_ERR_ARG
