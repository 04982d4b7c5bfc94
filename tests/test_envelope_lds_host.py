"""The envelope kernels' dynamic LDS layout (csrc/dkg_device.h env_lds) through dkg_debug_envelope_lds: the one
function the kernels carve their LDS by and the host sizes, streams and refuses by.  CPU only (host arithmetic).

(a) its total is, byte for byte, what the host's three former formulas gave (tests/envelope_lds_ref.py);
(b) its regions lie in the documented order, each at least its documented size, none overlapping,
    the last ending at the total, and the regions read as double2 or filled by 16-byte DMA pieces start on 16 bytes;
(c) bad arguments are DKG_ERR_ARG.
"""

import ctypes
import itertools

import pytest

import envelope_lds_ref as ref
from dkg_amd import _lib

REGIONS = ["pad", "lmu", "lcv", "lw", "skg", "sbuf", "cbuf", "sif", "sidx", "qrow", "jrow", "sgv", "sgm", "sgw", "sx",
           "sil", "shD", "suw", "sscl", "shk"]
NREG = 20
# (grad, stream, grows)
MODES = {
    "forward-staged": (0, 0, 0),
    "forward-stream": (0, 1, 0),
    "grad-staged": (1, 0, 0),
    "grad-stream": (1, 1, 0),
    "grad-rows": (1, 1, 1),
}
M_ALL = range(1, 9)
N_ALL = (0, 1, 63, 64, 127, 128, 511, 512, 1087, 1088, 2111, 2112, 5000)
WAVES_ALL = (1, 2, 4, 8)
S_ALL = (1, 7, 8, 9, 32)
D_ALL = (1, 2, 6, 16)
NP_ALL = (16, 256, 272, 1024)


def layout(m, N, waves, S, d, max_np, mode, out=None):
    out = out if out is not None else (ctypes.c_int * (NREG + 1))()
    st = _lib.load().dkg_debug_envelope_lds(m, N, waves, S, d, max_np, *mode, out)
    assert st == _lib.DKG_OK, (st, _lib.load().dkg_last_error())
    return list(out)


def ref_bytes(m, N, waves, S, d, max_np, mode):
    grad, stream, grows = mode
    if grows:
        return ref.envelope_grad_rows_lds_bytes(m, N, waves, S, max_np)
    if grad:
        return ref.envelope_grad_lds_bytes(m, N, waves, S, d, max_np, bool(stream))
    return ref.envelope_lds_bytes(m, N, waves, S, bool(stream))


def documented_sizes(m, N, waves, S, d, max_np, mode):
    """Doubles each region holds at least, None where the mode has no such region."""
    grad, stream, grows = mode
    M = ref.outputs_bucket(m)
    rec = ref.cov_rec(M)
    records = 0 if stream else max(ref.stage_len(N * rec), 64 * ref.env_slots(N + 1) * rec)
    LC = 512 if stream and not grad else 128
    rows = ref.stage_len(max_np)
    half = lambda ints: (ints + 1) // 2  # noqa: E731  (ints packed two to a double)
    sz = dict.fromkeys(REGIONS)
    sz.update(pad=8, lmu=0 if stream else records + 8, lcv=records, lw=S * m, skg=S, sbuf=waves * 2 * LC)
    if not grad:
        chunks = 4 * 8 * 64 * rec if 2 <= M <= 4 else 0
        sz.update(cbuf=max(waves * 192, chunks) if stream else 0, sif=half(waves * LC))
        return sz
    sz.update(sidx=half(waves * 128), sgv=M * 16, sgm=M * 16, sgw=waves * 64, sx=16, sil=M * 16, shD=waves * 128,
              suw=waves * max_np, sscl=waves * 128, shk=half(waves * 128))
    if not grows:
        sz.update(qrow=M * rows, jrow=M * d * rows)
    return sz


@pytest.mark.parametrize("mode", MODES)
def test_total_is_the_former_host_formula(mode):
    out = (ctypes.c_int * (NREG + 1))()
    for m, N, waves, S, d, max_np in itertools.product(M_ALL, N_ALL, WAVES_ALL, S_ALL, D_ALL, NP_ALL):
        got = layout(m, N, waves, S, d, max_np, MODES[mode], out)[NREG] * 8
        assert got == ref_bytes(m, N, waves, S, d, max_np, MODES[mode]), (mode, m, N, waves, S, d, max_np)


@pytest.mark.parametrize("mode", MODES)
def test_regions(mode):
    out = (ctypes.c_int * (NREG + 1))()
    for m, N, waves, S, d, max_np in itertools.product(M_ALL, N_ALL, WAVES_ALL, S_ALL, D_ALL, NP_ALL):
        point = (mode, m, N, waves, S, d, max_np)
        off = layout(m, N, waves, S, d, max_np, MODES[mode], out)
        total = off[NREG]
        size = documented_sizes(m, N, waves, S, d, max_np, MODES[mode])
        # the mode's regions, and no others
        assert [r for r, o in zip(REGIONS, off) if o >= 0] == [r for r in REGIONS if size[r] is not None], point
        present = [(r, o) for r, o in zip(REGIONS, off) if o >= 0]
        assert present[0] == ("pad", 0), point
        # documented order; each region's documented size ends at or before the next region's start (so none
        # overlap), the last one's exactly at the total
        ends = [o for _, o in present[1:]] + [total]
        for (r, o), end in zip(present, ends):
            assert o + size[r] <= end, (point, r)
        last, o = present[-1]
        assert o + size[last] == total, point
        for r in ("lmu", "lcv", "cbuf", "qrow", "jrow"):  # double2 reads / 16-byte DMA pieces
            if size[r] is not None:
                assert off[REGIONS.index(r)] % 2 == 0, (point, r)


def test_design_table_names_the_regions():
    """DESIGN.md 4.13's table lists the entry's regions, in its order, with the modes that have them."""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    table = text.split("<!-- env-lds-regions -->")[1].split("<!-- /env-lds-regions -->")[0]
    rows = re.findall(r"^\| `(\w+)` \|[^|]*\| ([^|]*) \|", table, re.M)
    assert [r for r, _ in rows] == REGIONS
    for mode in MODES.values():
        grad, _, grows = mode
        doc = [r for r, where in rows if where == "all" or (where.startswith("gradient") if grad else
                                                             where == "forward")]
        if grows:
            doc = [r for r in doc if r not in ("qrow", "jrow")]
        off = layout(2, 1024, 8, 16, 2, 256, mode)
        assert [r for r, o in zip(REGIONS, off) if o >= 0] == doc


GOOD = dict(m=2, N=1024, waves=8, S=16, d=2, max_np=256, grad=1, stream=1, grows=0)


@pytest.mark.parametrize("bad", [
    dict(m=0), dict(m=9), dict(N=-1), dict(N=(1 << 22) + 1), dict(waves=0), dict(waves=9), dict(S=0),
    dict(S=1 << 24, m=2), dict(d=0), dict(d=17), dict(max_np=0), dict(max_np=24), dict(max_np=1040),
    dict(grows=1, grad=0, stream=1), dict(grows=1, grad=1, stream=0), dict(grows=1, grad=0, stream=0),
], ids=str)
def test_bad_arguments(bad):
    lib = _lib.load()
    out = (ctypes.c_int * (NREG + 1))()
    a = dict(GOOD, **bad)
    args = [a[k] for k in ("m", "N", "waves", "S", "d", "max_np", "grad", "stream", "grows")]
    assert lib.dkg_debug_envelope_lds(*args, out) == _lib.DKG_ERR_ARG
    assert b"dkg_debug_envelope_lds" in lib.dkg_last_error()


def test_null_out_and_good_arguments():
    lib = _lib.load()
    args = [GOOD[k] for k in ("m", "N", "waves", "S", "d", "max_np", "grad", "stream", "grows")]
    assert lib.dkg_debug_envelope_lds(*args, None) == _lib.DKG_ERR_ARG
    out = (ctypes.c_int * (NREG + 1))()
    assert lib.dkg_debug_envelope_lds(*args, out) == _lib.DKG_OK
    assert lib.dkg_abi_version() == 9 == _lib.ABI_VERSION
