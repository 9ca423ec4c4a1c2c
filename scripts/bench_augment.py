"""The interpolated-sinc resampler against a copy and against the host path
(run on the GPU box):

  kernel  `resampy.resample` of 32 x 10 s on the device for the rate pairs of
          augmentation (48 000 -> 22 050, 54 441 -> 44 100, 22 050 -> 44 100,
          88 200 -> 44 100): device time between events over a warmed window
          of at least WINDOW seconds, median and spread of ROUNDS rounds;
  copy    a device-to-device copy that moves the same bytes (it reads and
          writes (input + output) / 2 bytes each), timed the same way in the
          same run;
  host    the host path of `resampy.resample` (numpy, one fma chain per
          output) on --host-rows rows of --host-seconds s, one row per thread
          of a pool of 16: wall time, and the time per output sample beside
          the kernel's. The host path is far too slow for the full shape.

Writes profiles/augment/bench.json (or --output). --quick: one short window
and no host run, for a profiler pass.
    python scripts/bench_augment.py
"""
import argparse
import concurrent.futures
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import promonet_amd  # noqa: E402,F401
from promonet_amd import resampy  # noqa: E402

ROUNDS, WINDOW = 5, .3
PAIRS = [(48000, 22050), (54441, 44100), (22050, 44100), (88200, 44100)]


def device_time(function, rounds=ROUNDS, window=WINDOW):
    """Median / min / max seconds per call of `function` over `rounds`
    windows of at least `window` seconds of device time"""
    for _ in range(3):
        function()
    torch.cuda.synchronize()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    calls, measured = 4, []
    while len(measured) < rounds:
        start.record()
        for _ in range(calls):
            function()
        end.record()
        end.synchronize()
        seconds = start.elapsed_time(end) * 1e-3
        if seconds < window:        # grow the window; the short one warmed
            calls = int(calls * max(2., 1.2 * window / max(seconds, 1e-6)))
            continue
        measured.append(seconds / calls)
    return {'median_us': statistics.median(measured) * 1e6,
            'min_us': min(measured) * 1e6, 'max_us': max(measured) * 1e6,
            'calls_per_round': calls, 'rounds': rounds}


def taps_per_output(orig, new):
    """Products of one output far from the row's ends: both wings"""
    step = min(orig, new) * resampy.STEPS // orig
    return 2 * (resampy.TABLE // step) - 1


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'augment' / 'bench.json'))
    parser.add_argument('--batch', type=int, default=32)
    parser.add_argument('--seconds', type=float, default=10.)
    parser.add_argument('--host-rows', type=int, default=16)
    parser.add_argument('--host-seconds', type=float, default=.5)
    parser.add_argument('--quick', action='store_true')
    parser.add_argument('--no-host', action='store_true')
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment.py needs the GPU')
    device = torch.device('cuda:0')
    rounds, window = (1, .05) if args.quick else (ROUNDS, WINDOW)
    results = {'device': torch.cuda.get_device_name(0), 'batch': args.batch,
               'seconds': args.seconds, 'host_threads': 16,
               'host_rows': args.host_rows,
               'host_seconds': args.host_seconds, 'workloads': {}}
    for orig, new in PAIRS:
        samples = int(orig * args.seconds)
        gen = torch.Generator().manual_seed(orig)
        host = torch.rand(args.batch, samples, generator=gen) * 2 - 1
        x = host.to(device)
        out = resampy.resample(x, orig, new)
        taps = taps_per_output(orig, new)
        moved = 4 * (x.numel() + out.numel())
        # two fmas a tap: the weight and the product
        flop = 4 * out.numel() * taps
        kernel = device_time(
            lambda: resampy.resample(x, orig, new), rounds, window)
        source = torch.empty(moved // 8, dtype=torch.float32, device=device)
        target = torch.empty_like(source)
        copy = device_time(lambda: target.copy_(source), rounds, window)
        entry = {
            'taps_per_output': taps, 'tile': resampy.tile(orig, new),
            'outputs': out.numel(), 'bytes_moved': moved, 'flop': flop,
            'kernel': kernel, 'copy_same_bytes': copy,
            'kernel_over_copy': kernel['median_us'] / copy['median_us'],
            'kernel_gflops': flop / kernel['median_us'] * 1e-3,
            'kernel_gtaps_per_s':
                out.numel() * taps / kernel['median_us'] * 1e-3,
            'kernel_ns_per_output':
                kernel['median_us'] * 1e3 / out.numel()}
        if not (args.quick or args.no_host):
            short = host[:args.host_rows, :int(orig * args.host_seconds)]
            times = []
            with concurrent.futures.ThreadPoolExecutor(16) as pool:
                for _ in range(2):
                    begin = time.perf_counter()
                    rows = list(pool.map(
                        lambda row: resampy.resample(row, orig, new), short))
                    times.append(time.perf_counter() - begin)
            want = torch.stack(rows)
            outputs = want.numel()
            entry.update({
                'host_runs_s': times, 'host_outputs': outputs,
                'host_ns_per_output': min(times) * 1e9 / outputs,
                'host_over_kernel_per_output':
                    min(times) * 1e9 / outputs /
                    entry['kernel_ns_per_output'],
                'device_equals_host': bool(torch.equal(
                    resampy.resample(short.to(device), orig, new).cpu(),
                    want))})
        results['workloads'][f'{orig}->{new}'] = entry
        print(json.dumps({f'{orig}->{new}': entry}), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
