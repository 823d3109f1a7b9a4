"""Slice sharding across ranks (one process per GPU).

Slices are independent units (one coder object each in the reference, recode.cpp:1270, 1525),
so the path shards with no data-path collective: rank r owns a contiguous range of slice
indices and generates / receives only those.  The only collectives are the ones the
measurement needs (barrier, max of the elapsed time, sum of the units).
"""
from __future__ import annotations


def shard_first_slice(rank: int, slices_per_rank: int) -> int:
    """Weak scaling: every rank processes `slices_per_rank` slices; rank r owns
    [r*slices_per_rank, (r+1)*slices_per_rank) of the global slice index space."""
    return rank * slices_per_rank


def lpt_assign(n_bins, world: int):
    """Greedy LPT: slices longest first, each to the rank with the least bins so far (ties: the lower rank).
    Returns the rank of every slice.  Same plan as avr_multi_submit (csrc/avr_multi.h) for slices that are their own units."""
    order = sorted(range(len(n_bins)), key=lambda i: -int(n_bins[i]))        # stable: equal lengths keep their order
    load = [0] * world
    owner = [0] * len(n_bins)
    for i in order:
        r = min(range(world), key=lambda k: load[k])
        owner[i] = r
        load[r] += int(n_bins[i])
    return owner


def lpt_assign_groups(n_bins, group_first, world: int):
    """Placement by units, the twin of avr::multi_place (csrc/avr_multi.h) for key records: group g holds the slices
    [group_first[g], group_first[g + 1]), the last one up to len(n_bins), and weighs the sum of their bins; a group without
    slices is no unit.  Groups heaviest first, equal weights in the caller's order, each to the rank with the least bins so far
    (ties: the lower rank).  Returns the rank of every slice: all slices of a group share one."""
    n = len(n_bins)
    bounds = [int(f) for f in group_first] + [n]
    units = [(bounds[g], bounds[g + 1]) for g in range(len(group_first)) if bounds[g] < bounds[g + 1]]
    weight = [sum(int(n_bins[i]) for i in range(a, b)) for a, b in units]
    order = sorted(range(len(units)), key=lambda u: -weight[u])           # stable
    load = [0] * world
    owner = [0] * n
    for u in order:
        r = min(range(world), key=lambda k: load[k])
        load[r] += weight[u]
        for i in range(*units[u]):
            owner[i] = r
    return owner


def balanced_ranges(n_bins, world: int):
    """Strong-scaling split into CONTIGUOUS slice ranges of near-equal bin totals (what a rank can generate from
    (seed, first_slice) alone): boundary r is where the running total comes closest to r/world of all bins.
    Returns world+1 non-decreasing boundaries, first 0, last len(n_bins)."""
    import numpy as np
    cum = np.cumsum(np.asarray(n_bins, dtype=np.int64))
    total = int(cum[-1]) if len(cum) else 0
    bounds = [0]
    for r in range(1, world):
        target = total * r / world
        i = int(np.searchsorted(cum, target, side="left"))            # cum[i] is the first total >= target
        if i < len(cum) and (i == 0 or abs(int(cum[i]) - target) <= abs(int(cum[i - 1]) - target)):
            i += 1                                                     # taking slice i too lands closer
        bounds.append(max(bounds[-1], min(i, len(cum))))
    bounds.append(len(cum))
    return bounds


def reduce_timing(dist, seconds: float, units: int, device):
    """(max over ranks of `seconds`, sum over ranks of `units`); identity without a process group."""
    if dist is None or not dist.is_available() or not dist.is_initialized():
        return float(seconds), int(units)
    import torch
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    u = torch.tensor([units], dtype=torch.int64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(u, op=dist.ReduceOp.SUM)
    return float(t.item()), int(u.item())
