"""Residency planning of the policy pool (host only; standard library): which of the up-to-MAX_SLOTS adapter slots holds which registered
policy, and which `(slot, name)` loads a batch needs before its forward.

Any number of policies stay registered (their tensors in device memory: engine.VLAEngine.pool_add); the slot storage the forward reads holds
`resident` of them.  A batch names at most `resident` distinct policies (predict_action_batch splits a longer list into passes).  Rules:
  * a needed policy that is already resident is never moved;
  * a missing one evicts the least recently used slot that the batch does not need; among equally old slots (never used, or emptied by
    pool_remove -- those are the oldest of all) the lowest slot goes first;
  * the result depends on nothing but (resident names, last-use ticks, needed names in order): deterministic.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

EMPTY_TICK = -1   # a slot that holds nothing (never loaded, or its policy was removed): older than anything that was ever used


def plan_loads(resident: Sequence[Optional[str]], last_used: Sequence[int], needed: Sequence[str]) -> List[Tuple[int, str]]:
    """resident[s]: the policy in slot s (None: empty or stale); last_used[s]: the tick of the last batch that needed slot s; needed: the
    distinct policies of one batch, in order of first appearance.  -> the (slot, name) loads to perform, in that order."""
    needed = list(needed)
    if len(set(needed)) != len(needed):
        raise ValueError(f"plan_loads: the needed policies {needed} are not distinct")
    if len(needed) > len(resident):
        raise ValueError(f"plan_loads: {len(needed)} distinct policies for {len(resident)} resident slots (split the batch into passes)")
    if len(last_used) != len(resident):
        raise ValueError("plan_loads: one last-use tick per slot")
    if any(n is None for n in needed):
        raise ValueError("plan_loads: a needed policy has no name")
    keep = {s for s, name in enumerate(resident) if name is not None and name in needed}
    have = {resident[s] for s in keep}
    free = sorted((s for s in range(len(resident)) if s not in keep), key=lambda s: (EMPTY_TICK if resident[s] is None else last_used[s], s))
    loads = []
    for name in needed:
        if name not in have:
            loads.append((free.pop(0), name))
    return loads


class Residency:
    """The pool's slot table and counters.  `stats`: loads (slot swaps performed), hits (needed policies found resident), passes (forwards)."""

    def __init__(self, resident: int):
        if resident < 1:
            raise ValueError(f"Residency: {resident} resident slots")
        self.names: List[Optional[str]] = [None] * resident
        self.last_used: List[int] = [EMPTY_TICK] * resident
        self.tick = 0
        self.stats: Dict[str, int] = dict(loads=0, hits=0, passes=0)

    def plan(self, needed: Sequence[str]) -> List[Tuple[int, str]]:
        return plan_loads(self.names, self.last_used, needed)

    def commit(self, loads: Sequence[Tuple[int, str]], needed: Sequence[str]) -> Dict[str, int]:
        """The loads of plan(needed) have been performed: one pass is counted, the needed slots become the most recently used.
        -> {name: slot} for the needed policies."""
        for s, name in loads:
            self.names[s] = name
        self.tick += 1
        slot_of = {}
        for name in needed:
            s = self.names.index(name)
            self.last_used[s] = self.tick
            slot_of[name] = s
        self.stats["loads"] += len(loads)
        self.stats["hits"] += len(needed) - len(loads)
        self.stats["passes"] += 1
        return slot_of

    def invalidate(self, name: str) -> Optional[int]:
        """`name` was removed from the pool: its slot (if it had one) is empty and stale -- never a hit again, first to be refilled."""
        if name not in self.names:
            return None
        s = self.names.index(name)
        self.names[s], self.last_used[s] = None, EMPTY_TICK
        return s


def split_passes(policies: Sequence[str], resident: int) -> List[List[str]]:
    """The distinct names of `policies` in order of first appearance, in groups of at most `resident`: one forward pass each."""
    distinct = list(dict.fromkeys(policies))
    return [distinct[i:i + resident] for i in range(0, len(distinct), resident)]
