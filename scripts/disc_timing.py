"""The timing loop of bench_fdisc.py, bench_dconv.py and bench_pconv.py (they
run from this directory, which is then on the path)."""
import statistics

import torch

ROUNDS = 7


def timed(functions, calls):
    """Interleaved: every round times each function once, `calls` calls"""
    for function in functions.values():
        function()
    torch.cuda.synchronize()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    rounds = {name: [] for name in functions}
    for _ in range(ROUNDS):
        for name, function in functions.items():
            start.record()
            for _ in range(calls):
                function()
            end.record()
            end.synchronize()
            rounds[name].append(start.elapsed_time(end) * 1e3 / calls)
    return {name: {'median_us': statistics.median(r), 'min_us': min(r),
                   'max_us': max(r), 'calls_per_round': calls}
            for name, r in rounds.items()}
