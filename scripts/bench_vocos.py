"""Benchmark the Vocos mel vocoder (MelGenerator at config/baselines/vocos.py)
on batch 32 x 861 frames (10 s utterances) for each operand type and print one
JSON line: ms per batch (HIP events, after warmup), M samples/s, TFLOP/s
against the 0.841 TFLOP of the batch, the fraction of the matching dense MFMA
peak, and - with --profile - per-kernel times of a `rocprofv3 --kernel-trace
--stats` run of this script in a child process.

    python scripts/bench_vocos.py [--steps 20] [--warmup 5] [--profile]

--ragged measures what a ragged batch (`MelGenerator.forward(..., lengths=)`)
costs. For each operand type, in one process, warmed, the variants alternated
over --rounds rounds and the median round kept:
  a  uniform 32 x 861 (the figure above)
  b  ragged: 32 utterances, lengths uniform in [215, 861] from a fixed seed,
     R = sum(lengths) packed rows
  c  uniform 32 x round(R / 32): the same rows to within 16
  c2 c again: |c2 / c - 1| over the rounds is the run-to-run spread
b / c is the cost of raggedness itself, b / a shows that time follows R. With
--profile, one rocprofv3 kernel-trace run each of b and of c.

    python scripts/bench_vocos.py --ragged [--rounds 5] [--profile]
"""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, FRAMES = 32, 861
FLOP = 0.841e12                      # 30.5 MFLOP a frame x 32 x 861
PEAK = {'fp32': 157e12, 'f16': 2.5e15, 'bf16': 2.5e15}
DTYPES = ('fp32', 'f16', 'bf16')


def ragged_lengths():
    import torch
    gen = torch.Generator().manual_seed(0)
    return torch.randint(215, FRAMES + 1, (BATCH,), generator=gen).tolist()


def make_model(dtype):
    import torch
    import promonet_amd
    promonet_amd.configure(
        MODEL='vocos', SPECTROGRAM_ONLY=True, AUGMENT_PITCH=False,
        AUGMENT_LOUDNESS=False, VOCOS_LAYERS=8, COMPUTE_DTYPE=dtype)
    torch.manual_seed(0)
    device = torch.device('cuda:0')
    return promonet_amd.model.MelGenerator().to(device).eval(), device


def workloads(model, device):
    """name -> a call running one batch of workload a, b or c"""
    import torch
    import promonet_amd
    lengths = ragged_lengths()
    rows = sum(lengths)
    speakers = torch.arange(BATCH, device=device) % promonet_amd.NUM_SPEAKERS
    ones = torch.ones(BATCH, device=device)
    full = torch.rand(BATCH, 513, FRAMES, device=device) + 1e-3
    same_rows = full[:, :, :round(rows / BATCH)].contiguous()
    on_device = torch.tensor(lengths, dtype=torch.int32, device=device)
    return rows, {
        'a': lambda: model(full, speakers, ones, ones),
        'b': lambda: model(full, speakers, ones, ones, lengths=on_device),
        'c': lambda: model(same_rows, speakers, ones, ones)}


def timed(call, steps):
    import torch
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def measure_ragged(dtype, steps, warmup, rounds):
    import statistics
    import torch
    model, device = make_model(dtype)
    rows, calls = workloads(model, device)
    order = ('a', 'b', 'c', 'c2')
    calls['c2'] = calls['c']
    times = {name: [] for name in order}
    with torch.inference_mode():
        for name in order:
            for _ in range(warmup):
                calls[name]()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name in order:
                times[name].append(timed(calls[name], steps))
    ms = {name: statistics.median(times[name]) for name in order}
    spread = max(abs(y / x - 1) for x, y in zip(times['c'], times['c2']))
    return {'rows': rows, 'rows_fraction': round(rows / (BATCH * FRAMES), 4),
            'uniform_frames_c': round(rows / BATCH),
            'a_ms': round(ms['a'], 4), 'b_ms': round(ms['b'], 4),
            'c_ms': round(ms['c'], 4), 'c2_ms': round(ms['c2'], 4),
            'b_over_c': round(ms['b'] / ms['c'], 4),
            'c_spread': round(spread, 4),
            'b_over_a': round(ms['b'] / ms['a'], 4),
            'rounds_ms': {name: [round(t, 4) for t in times[name]]
                          for name in order}}


def run_workload(name, dtype, steps, warmup):
    """(under rocprofv3) warmup + steps batches of one workload"""
    import torch
    model, device = make_model(dtype)
    _, calls = workloads(model, device)
    with torch.inference_mode():
        for _ in range(warmup + steps):
            calls[name]()
        torch.cuda.synchronize()


def measure(dtype, steps, warmup):
    import torch
    import promonet_amd
    model, device = make_model(dtype)
    spectrograms = torch.rand(BATCH, 513, FRAMES, device=device) + 1e-3
    speakers = torch.arange(BATCH, device=device) % promonet_amd.NUM_SPEAKERS
    ones = torch.ones(BATCH, device=device)
    with torch.inference_mode():
        for _ in range(warmup):
            model(spectrograms, speakers, ones, ones)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            model(spectrograms, speakers, ones, ones)
        end.record()
        torch.cuda.synchronize()
    ms = start.elapsed_time(end) / steps
    return {'ms_per_batch': round(ms, 4),
            'msamples_per_s': round(BATCH * FRAMES * 256 / ms / 1e3, 2),
            'tflops': round(FLOP / ms / 1e9, 2),
            'fraction_of_mfma_peak': round(FLOP / (ms * 1e-3) / PEAK[dtype],
                                           4)}


def profile(steps, warmup, workload=None):
    """per-kernel totals (ms a batch) of one rocprofv3 kernel-trace run"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run(
            ['rocprofv3', '--kernel-trace', '--stats', '--output-format',
             'csv', '-d', tmp, '-o', 'vocos', '--', sys.executable,
             __file__, '--inner', '--steps', str(steps), '--warmup',
             str(warmup)] + (['--workload', workload] if workload else []),
            capture_output=True, text=True, timeout=900)
        if done.returncode != 0:
            return {'error': done.stderr[-500:]}
        files = list(Path(tmp).rglob('*kernel_stats.csv'))
        if not files:
            return {'error': 'no kernel_stats.csv'}
        # every dtype runs warmup + steps forwards: a kernel templated on the
        # operand type (Elem*) serves one dtype, the others all three
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row['Name'].split('(')[0]
                calls = (steps + warmup) * (1 if 'Elem' in name else
                                            len(DTYPES))
                out[name[:80]] = round(
                    float(row['TotalDurationNs']) / 1e6 / calls, 4)
    return dict(sorted(out.items(), key=lambda kv: -kv[1])[:24])


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=5)
    parser.add_argument('--profile', action='store_true')
    parser.add_argument('--dtypes', default=','.join(DTYPES),
                        help='comma-separated subset of fp32,f16,bf16')
    parser.add_argument('--ragged', action='store_true',
                        help='the cost of a ragged batch (see above)')
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--inner', action='store_true',
                        help=argparse.SUPPRESS)
    parser.add_argument('--workload', choices=('a', 'b', 'c'),
                        help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.workload:
        for dtype in args.dtypes.split(','):
            run_workload(args.workload, dtype, args.steps, args.warmup)
        return
    if args.ragged:
        result = {'metric': 'vocos_ragged_batch', 'batch': BATCH,
                  'frames': FRAMES, 'lengths': ragged_lengths()}
        for dtype in args.dtypes.split(','):
            result[dtype] = measure_ragged(
                dtype, args.steps, args.warmup, args.rounds)
        if args.profile:
            for name in ('b', 'c'):
                result[f'kernels_ms_per_batch_{name}'] = profile(
                    args.steps, args.warmup, name)
        print(json.dumps(result))
        return
    result = {'metric': 'vocos_mel_vocoder', 'batch': BATCH,
              'frames': FRAMES, 'tflop_per_batch': FLOP / 1e12}
    for dtype in args.dtypes.split(','):
        result[dtype] = measure(dtype, args.steps, args.warmup)
    if args.profile and not args.inner:
        result['kernels_ms_per_batch'] = profile(
            args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
