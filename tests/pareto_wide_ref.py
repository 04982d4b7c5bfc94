"""Inputs and closed-form expectations for the wide rank path's tests (test infrastructure, not a test).

* ``cut_to_keep``: ``dkg_pareto_rank``'s result for any ``keep`` from its result for ``keep = Q``.  The header's
  rule: fronts in order until at least ``keep`` points are ranked, the last front whole; the others get rank -1 and
  crowding 0 and leave ``order``.  A ranked front's crowding does not depend on the fronts after it.
* ``tiled_input`` / ``tiled_expected``: ``F[i] = base[i % B] + 4 (i // B)`` for a base of B points with coordinates
  that are multiples of 2^-10 in [0, 1).  Every coordinate of block b exceeds every coordinate of the blocks below,
  so block b dominates them all and fronts never span blocks; sums and differences of such numbers below 1024 are
  exact, so a block's crowding has the base's bits.  With ``nb`` blocks:
  rank = (nb - 1 - block) fronts(base) + rank_base, crowding the base's, order by block descending then the base's.
"""

import numpy as np

import pareto_ref


def cut_to_keep(rank, crowd, order, keep):
    """(rank, crowd, order) for ``keep`` from the fully ranked (keep = Q) result."""
    rank = np.asarray(rank)
    sizes = np.bincount(rank, minlength=int(rank.max()) + 1)
    nfronts = int(np.searchsorted(np.cumsum(sizes), keep)) + 1  # the first front at which keep points are ranked
    on = rank < nfronts
    r = np.where(on, rank, -1).astype(np.int32)
    c = np.where(on, crowd, 0.0)
    o = np.full(rank.size, -1, dtype=np.int32)
    kept = np.asarray(order)[: int(on.sum())]  # order lists fronts in rank order: the kept ones come first
    o[: kept.size] = kept
    return r, c, o


def tiled_base(B=64, m=2, seed=5):
    g = np.random.default_rng(seed)
    return g.integers(0, 1024, size=(B, m)).astype(np.float64) / 1024.0


def tiled_input(base, nb):
    B = base.shape[0]
    i = np.arange(B * nb)
    return base[i % B] + 4.0 * (i // B)[:, None]


def tiled_expected(base, nb, keep):
    """The closed form; only ``rank_crowd_order(base)`` is computed."""
    B = base.shape[0]
    rb, cb, ob = pareto_ref.rank_crowd_order(base)
    fronts = int(rb.max()) + 1
    block = np.arange(B * nb) // B
    rank = ((nb - 1 - block) * fronts + np.tile(rb, nb)).astype(np.int32)
    crowd = np.tile(cb, nb)
    order = np.concatenate([ob.astype(np.int64) + B * b for b in range(nb - 1, -1, -1)]).astype(np.int32)
    return cut_to_keep(rank, crowd, order, keep)
