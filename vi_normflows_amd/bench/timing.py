"""HIP-event timing shared by the kernel benchmarks of this package."""
from __future__ import annotations

import statistics

import torch


def event_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0


def alternate(fns: dict, reps: int, warmup: int = 3) -> dict:
    """Median us of each callable, the callables taking turns rep by rep. A callable marked
    ``self_timed`` returns its own event time (it has untimed set-up of its own)."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(f() if getattr(f, "self_timed", False) else event_us(f))
    return {k: statistics.median(v) for k, v in t.items()}
