"""Shared by the transform plans' test_stage_times cases: the timing ring grown
and shrunk between runs of one plan."""
from __future__ import annotations

import math

# (slots, runs): more runs than slots each time, a larger ring, then a smaller one
PHASES = ((2, 3), (4, 5), (1, 2))


def check_ring_phases(plan, rerun, names):
    """rerun(): one more complete run of `plan`, synchronised.  After each phase
    stage_times() has exactly `names`, in order, every value finite and
    positive, and "total" no smaller than any stage."""
    for slots, runs in PHASES:
        plan.set_timing(slots)
        for _ in range(runs):
            rerun()
        t = plan.stage_times()
        assert list(t) == list(names), (slots, t)
        assert all(math.isfinite(v) and v > 0 for v in t.values()), (slots, t)
        assert all(t["total"] >= v for v in t.values()), (slots, t)
