"""The LPC feature kernel (pm_harmonics_lpc) on 32 x 10 s, beside a copy of
the same bytes and the CPU oracle on the same host (run on the GPU box):

  kernel  `preprocess.harmonics.lpc` on (32, 220 500) samples: device time
          between events, median / min / max of ROUNDS rounds of CALLS calls;
  copy    a device-to-device copy of HALF the bytes the kernel reads and
          writes (audio in + features out): it reads that half and writes it,
          so it moves as many bytes as the kernel does; timed the same way
          in the same run: the floor of anything that touches those bytes;
  oracle  tests/lpc_oracle.py, the literal float32 recursion and the response
          frame by frame in the reference's call pattern, on ONE 10 s
          recording over 16 worker processes: wall time. It is this oracle's
          time (numpy, a fixed summation tree), not the reference's numba
          routine's. The batch figure is that time x 32: EXTRAPOLATED, not
          run.

Prints one JSON line and writes profiles/lpc/bench.json (or --output).
    python scripts/bench_lpc.py
"""
import argparse
import json
import multiprocessing
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
import promonet_amd  # noqa: E402
from promonet_amd.preprocess import harmonics  # noqa: E402
import lpc_oracle as oracle  # noqa: E402

ROUNDS = 7
CALLS = 20
WORKERS = 16


def device_time(function, calls=CALLS):
    """Median / min / max microseconds per call over ROUNDS rounds"""
    function()
    torch.cuda.synchronize()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    rounds = []
    for _ in range(ROUNDS):
        start.record()
        for _ in range(calls):
            function()
        end.record()
        end.synchronize()
        rounds.append(start.elapsed_time(end) * 1e3 / calls)
    return {'median_us': statistics.median(rounds), 'min_us': min(rounds),
            'max_us': max(rounds), 'calls_per_round': calls}


def oracle_frame(frame):
    a = oracle.burg(frame, oracle.ORDER, np.float32)
    return np.log10(oracle.response(a))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'lpc' / 'bench.json'))
    parser.add_argument('--seconds', type=float, default=10.)
    parser.add_argument('--batch', type=int, default=32)
    args = parser.parse_args()
    samples = int(args.seconds * promonet_amd.SAMPLE_RATE)
    voice = oracle.resonant(
        (700., 1800., 3200.), (90., 110., 150.), 40., samples, 1)

    # the oracle first: its workers are forked before the GPU is opened
    windowed = oracle.frames(voice, np.float32)
    begin = time.perf_counter()
    with multiprocessing.Pool(WORKERS) as pool:
        want = np.stack(pool.map(oracle_frame, list(windowed), chunksize=8))
    oracle_us = (time.perf_counter() - begin) * 1e6

    if not torch.cuda.is_available():
        raise SystemExit('bench_lpc.py needs the GPU')
    device = torch.device('cuda:0')
    audio = torch.from_numpy(voice)[None].repeat(args.batch, 1).to(device)
    out = harmonics.lpc(audio)
    torch.cuda.synchronize()
    count = harmonics.lpc_frames(samples)
    assert out.shape == (args.batch, count, 512) and len(want) == count
    assert torch.equal(out[0], out[-1])
    difference = float(np.abs(
        out[0].cpu().numpy().astype(np.float64) - want).max())

    moved = audio.numel() * 4 + out.numel() * 4
    source = torch.empty(moved // 2, dtype=torch.uint8, device=device)
    target = torch.empty_like(source)
    kernel = device_time(lambda: harmonics.lpc(audio))
    copy = device_time(lambda: target.copy_(source))
    kernel_again = device_time(lambda: harmonics.lpc(audio))
    results = {
        'device': torch.cuda.get_device_name(0),
        'batch': args.batch, 'seconds': args.seconds, 'samples': samples,
        'frames': args.batch * count, 'order': oracle.ORDER,
        'bytes_in': audio.numel() * 4, 'bytes_out': out.numel() * 4,
        'kernel': kernel, 'kernel_second_pass': kernel_again, 'copy': copy,
        'copy_bytes_read_plus_written': 2 * (moved // 2),
        'kernel_over_copy': kernel['median_us'] / copy['median_us'],
        'kernel_ns_per_frame':
            kernel['median_us'] * 1e3 / (args.batch * count),
        'oracle': 'tests/lpc_oracle.py (numpy), float32, per frame',
        'oracle_one_recording_us': oracle_us, 'oracle_workers': WORKERS,
        'oracle_batch_us_extrapolated': oracle_us * args.batch,
        'device_vs_float32_oracle_max': difference}
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
