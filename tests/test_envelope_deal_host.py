"""The envelope launches' map from workgroup id to (item, member) (csrc/dkg_common.h xcd_deal) through
dkg_debug_envelope_deal: the arithmetic the kernels run, on the host.  A launch over `nitems` items of `groups`
workgroups each has 8 * groups * ceil(nitems / 8) ids; ids L and L + 8 share an XCD.  CPU only.
"""
import ctypes

import pytest

from dkg_amd import _lib


def _deal(lib, L, nitems, groups):
    item, member = ctypes.c_int(-1), ctypes.c_int(-1)
    st = lib.dkg_debug_envelope_deal(L, nitems, groups, ctypes.byref(item), ctypes.byref(member))
    return st, item.value, member.value


def _size(nitems, groups):
    return 8 * groups * ((nitems + 7) // 8)


@pytest.mark.parametrize("groups", range(1, 7))
def test_every_item_member_exactly_once_and_members_side_by_side(groups):
    lib = _lib.load()
    for nitems in range(1, 201):
        where = {}
        for L in range(_size(nitems, groups)):
            st, item, member = _deal(lib, L, nitems, groups)
            assert st in (0, 1)
            assert 0 <= member < groups
            if st == 0:
                assert item >= nitems  # a padding id never names a real item
                continue
            assert 0 <= item < nitems
            assert (item, member) not in where, f"({item}, {member}) twice, nitems={nitems}"
            where[item, member] = L
        assert len(where) == nitems * groups
        for item in range(nitems):
            ids = [where[item, g] for g in range(groups)]
            assert len({L & 7 for L in ids}) == 1  # one XCD
            assert [L >> 3 for L in ids] == list(range(ids[0] >> 3, (ids[0] >> 3) + groups))  # consecutive, in order
            assert (ids[0] & 7) == (item + item // 8 + item // 64) % 8


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("first", [0, 512, 1536])
def test_every_residue_takes_every_index_pattern_once_in_512_items(groups, first):
    """Over an aligned 512 items, each launch residue takes each (item % 8, (item / 8) % 8) exactly once: neither
    the index's lowest three bits nor the next three can line up with the hardware's modulo 8."""
    lib = _lib.load()
    nitems = first + 512
    seen = {r: [] for r in range(8)}
    for L in range(_size(first, groups) if first else 0, _size(nitems, groups)):
        st, item, member = _deal(lib, L, nitems, groups)
        assert st == 1 and first <= item < nitems
        if member == 0:
            seen[L & 7].append((item % 8, (item // 8) % 8))
    for r in range(8):
        assert sorted(seen[r]) == [(i, j) for i in range(8) for j in range(8)]


def test_arguments():
    lib = _lib.load()
    item, member = ctypes.c_int(0), ctypes.c_int(0)
    bad = [(-1, 8, 1), (8, 8, 1), (16, 9, 1), (0, 0, 1), (0, 1, 0), (0, 1 << 30, 8)]
    for L, nitems, groups in bad:
        assert lib.dkg_debug_envelope_deal(L, nitems, groups, ctypes.byref(item), ctypes.byref(member)) == -2
        assert b"dkg_debug_envelope_deal" in lib.dkg_last_error()
    assert lib.dkg_debug_envelope_deal(0, 1, 1, None, ctypes.byref(member)) == -2
    assert lib.dkg_debug_envelope_deal(0, 1, 1, ctypes.byref(item), None) == -2
    assert lib.dkg_debug_envelope_deal(0, 1, 1, ctypes.byref(item), ctypes.byref(member)) == 1
    assert (item.value, member.value) == (0, 0)
    assert lib.dkg_debug_envelope_deal(15, 9, 1, ctypes.byref(item), ctypes.byref(member)) in (0, 1)
