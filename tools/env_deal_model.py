"""Where the envelope launch's walked pairs land on the chip, from the CPU oracle alone (no GPU, no library).

usage: python tools/env_deal_model.py [workload] [--batches 5 32] [--costs 1.8 2.5] [--seed 0]

The envelope stage is the one whose work depends on the data: a (candidate, scalarisation) pair that fails the
flat test (csrc/dkg_device.h env_flat) is filtered and walked, and its workgroup (8 waves, one pair each, which
meet at a barrier) lasts 2-3 times as long as a workgroup of flat pairs.  Workgroup ids are dealt round-robin over
the 8 XCDs, so which launch residue (id % 8) an item gets decides which XCD runs it.  This tool

 * builds the lines of every pair of the workload with oracle.discretekg.lines_batched and applies env_flat's
   test, fma(48, |b - b_T|, a - a_T) <= 2^-40 (a - a_T) for every line, T = the top line (max a, then min b);
 * counts, per launch residue, the workgroups that hold a walked pair under three maps: xcd_group's (item b on
   residue b % 8), one rotation ((b + b / 8) % 8) and xcd_deal's ((b + b / 8 + b / 64) % 8, csrc/dkg_common.h);
 * list-schedules every residue's workgroups, in launch order, onto the 64 places of an XCD (32 CUs x 2 workgroups)
   with a flat workgroup costing 1 and a walked one `cost`, and prints the launch length (the longest XCD) per
   map beside a perfect balance (the summed cost / 512 places).

The costs are guesses that bracket the pair stamps (tools/pair_stamps.py): the model ranks maps for a candidate
set, it does not predict microseconds.
"""
import argparse
import heapq
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]

import torch  # noqa: E402

ENV_FLAT_Z = 48.0
ENV_FLAT_REL = 2.0 ** -40
PLACES = 64  # workgroups resident on one XCD: 32 CUs x 2 eight-wave workgroups

MAPS = {
    "b % 8": lambda b: b % 8,
    "(b + b/8) % 8": lambda b: (b + b // 8) % 8,
    "(b + b/8 + b/64) % 8": lambda b: (b + b // 8 + b // 64) % 8,
}


def flat_pairs(workload, seed=0, target=None):
    """bool [B, S]: the pairs of the workload's batch that env_flat settles without a walk."""
    from dkg_amd.synthetic import WORKLOADS, make_problem
    from oracle.discretekg import lines_batched
    from oracle.gp import ModelList, OutputGP

    w = WORKLOADS[workload] if isinstance(workload, str) else workload
    model, D, X, W = make_problem(w, seed)
    om = ModelList([OutputGP(m.train_x, m.train_y, m.lengthscale, m.outputscale, m.noise, m.mean_constant,
                             m.kernel, m.nu, m.y_mean, m.y_std) for m in model.models])
    a, b = lines_batched(om, X, D, W, target)
    return flat_from_lines(a, b)


def flat_from_lines(a, b):
    """env_flat on lines a, b [B, S, N + 1] (fp64; the fma is emulated by a plain multiply-add: the test's margin
    of 2^-40 is far above one rounding)."""
    aT = a.max(-1, keepdim=True).values
    bT = torch.where(a == aT, b, torch.full_like(b, float("inf"))).min(-1, keepdim=True).values
    da = a - aT
    worst = (ENV_FLAT_Z * (b - bT).abs() + da - ENV_FLAT_REL * da).max(-1).values
    return ~(worst > 0.0)


def walked_workgroups(flat, waves=8):
    """bool [B, groups]: the workgroups (candidate, group of `waves` consecutive pairs) with a walked pair."""
    B, S = flat.shape
    groups = (S + waves - 1) // waves
    pad = torch.ones(B, groups * waves, dtype=torch.bool)
    pad[:, :S] = flat
    return ~pad.view(B, groups, waves).all(-1)


def residue_counts(walked, residue):
    """Workgroups with a walked pair per launch residue, and all workgroups per residue."""
    B, groups = walked.shape
    hit, tot = [0] * 8, [0] * 8
    for b in range(B):
        r = residue(b)
        hit[r] += int(walked[b].sum())
        tot[r] += groups
    return hit, tot


def launch_length(walked, batches, residue, cost):
    """The longest XCD of a launch of `batches` copies of the batch: every residue's workgroups, in launch order
    (item order within the residue, an item's members one after another), list-scheduled onto PLACES places."""
    B, groups = walked.shape
    queues = [[] for _ in range(8)]
    for item in range(batches * B):
        q = queues[residue(item)]
        for g in range(groups):
            q.append(cost if walked[item % B, g] else 1.0)
    longest = 0.0
    for q in queues:
        free = [0.0] * PLACES
        heapq.heapify(free)
        end = 0.0
        for c in q:
            t = heapq.heappop(free) + c
            end = max(end, t)
            heapq.heappush(free, t)
        longest = max(longest, end)
    return longest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="headline")
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--costs", type=float, nargs="+", default=[1.8, 2.5])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    flat = flat_pairs(args.workload, args.seed)
    walked = walked_workgroups(flat)
    B, groups = walked.shape
    print(f"{args.workload}: {int((~flat).sum())} pairs fail the flat test ({int(flat.sum())} flat), in "
          f"{int((~flat).any(-1).sum())} of {B} candidates and {int(walked.sum())} of {B * groups} workgroups")
    for name, residue in MAPS.items():
        hit, tot = residue_counts(walked, residue)
        print(f"  workgroups with a walked pair per residue, {name:22s}: {hit} of {tot}")
    print("launch length, list-scheduled (flat workgroup = 1):")
    print(f"  {'batches':>7s} {'walked':>6s} " + " ".join(f"{n:>22s}" for n in MAPS) + f" {'perfectly balanced':>20s}")
    for K in args.batches:
        for cost in args.costs:
            lens = [launch_length(walked, K, residue, cost) for residue in MAPS.values()]
            total = K * (float(walked.sum()) * cost + float((~walked).sum()))
            print(f"  {K:7d} {cost:6.1f} " + " ".join(f"{v:22.1f}" for v in lens) + f" {total / (8 * PLACES):20.1f}")


if __name__ == "__main__":
    main()
