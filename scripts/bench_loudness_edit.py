"""The device limiter, shift and scale against a copy (run on the GPU box):

  limit   `loudness.limit` of 32 x 220 500 samples (10 s) on three inputs:
          quiet (uniform in +-0.98), speech-like (sigma .2 with one 20-sample
          burst above the threshold every second) and saturated (|x| uniform
          in [1, 4]); with each, what the kernel counted: the steps one lane
          walked serially (envelope carries, gain) and the tiles it skipped;
  copy    a device-to-device copy of the bytes `limit` reads and writes;
  shift   `loudness.shift` with a contour of 861 frames, and `loudness.scale`.

Device time between events; the workloads take turns inside each of ROUNDS
rounds, and the median over the rounds is reported. The CPU column is the
literal loop of tests/loudness_edit_oracle.py on 3 000 samples of one row,
EXTRAPOLATED to the row (the loop is linear in the samples).

Writes profiles/loudness_edit/bench.json (or --output).
    python scripts/bench_loudness_edit.py
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
import promonet_amd  # noqa: E402
from promonet_amd.preprocess import loudness  # noqa: E402

ROUNDS, WINDOW = 7, .05


def inputs(batch, samples):
    gen = torch.Generator().manual_seed(114)
    quiet = torch.rand(batch, samples, generator=gen) * 1.96 - .98
    speech = torch.randn(batch, samples, generator=gen) * .2
    speech = speech.clamp(-.98, .98)
    for start in range(promonet_amd.SAMPLE_RATE // 2, samples - 20,
                       promonet_amd.SAMPLE_RATE):
        speech[:, start:start + 20] *= 8
    sign = torch.where(torch.rand(batch, samples, generator=gen) < .5, -1., 1.)
    saturated = (1 + 3 * torch.rand(batch, samples, generator=gen)) * sign
    return {'quiet': quiet, 'speech_like': speech, 'saturated': saturated}


def calls_for(function):
    """Calls that fill a window of WINDOW seconds of device time (warms too)"""
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for _ in range(2):
        function()
    calls = 1
    while True:
        start.record()
        for _ in range(calls):
            function()
        end.record()
        end.synchronize()
        seconds = start.elapsed_time(end) * 1e-3
        if seconds >= WINDOW or calls >= 4096:
            return calls
        calls = max(calls + 1, int(calls * 1.2 * WINDOW / max(seconds, 1e-6)))


def interleaved(workloads):
    """name -> statistics of the seconds per call, the workloads taking turns
    in every round"""
    calls = {name: calls_for(f) for name, f in workloads.items()}
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    rounds = {name: [] for name in workloads}
    for _ in range(ROUNDS):
        for name, function in workloads.items():
            start.record()
            for _ in range(calls[name]):
                function()
            end.record()
            end.synchronize()
            rounds[name].append(start.elapsed_time(end) * 1e-3 / calls[name])
    return {name: {'median_us': statistics.median(r) * 1e6,
                   'min_us': min(r) * 1e6, 'max_us': max(r) * 1e6,
                   'calls_per_round': calls[name], 'rounds': ROUNDS}
            for name, r in rounds.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--output', default=str(
        ROOT / 'profiles' / 'loudness_edit' / 'bench.json'))
    parser.add_argument('--batch', type=int, default=32)
    parser.add_argument('--samples', type=int, default=220500)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_loudness_edit.py needs the GPU')
    import loudness_edit_oracle as oracle
    device = torch.device('cuda:0')
    batch, samples = args.batch, args.samples
    host = inputs(batch, samples)
    on_device = {name: x.to(device) for name, x in host.items()}
    frames = samples // promonet_amd.HOPSIZE
    gen = torch.Generator().manual_seed(861)
    contour = (torch.rand(batch, frames, generator=gen) * 12 - 6).to(device)
    target = (torch.rand(batch, 8, frames, generator=gen) * 20 - 50).to(device)
    source = torch.empty(batch, samples, device=device)
    sink = torch.empty_like(source)
    chunk, tile = loudness.limit_tile()
    results = {
        'device': torch.cuda.get_device_name(0), 'batch': batch,
        'samples': samples, 'frames': frames, 'chunk': chunk, 'tile': tile,
        'bytes_read_and_written': 8 * batch * samples, 'limit': {}}

    workloads = {'copy': lambda: sink.copy_(source)}
    for name, x in on_device.items():
        workloads[f'limit/{name}'] = lambda x=x: loudness.limit(x)
    speech = on_device['speech_like']
    workloads['shift'] = lambda: loudness.shift(speech, contour)
    workloads['scale'] = lambda: loudness.scale(speech, target)
    workloads['from_audio'] = lambda: loudness.from_audio(speech)
    timed = interleaved(workloads)
    results['copy'] = timed['copy']
    for name in ('shift', 'scale', 'from_audio'):
        results[name] = timed[name]
        results[name]['over_copy'] = \
            timed[name]['median_us'] / timed['copy']['median_us']

    for name, x in on_device.items():
        out, _, counts = loudness.limit_with_trace(x)
        counts = counts.cpu().to(torch.float64)
        piece = host[name][:1, :3000]
        times = []
        for _ in range(3):
            begin = time.perf_counter()
            want, _ = oracle.limit_literal(piece)
            times.append(time.perf_counter() - begin)
        assert torch.equal(
            loudness.limit(piece.to(device)).cpu(), want), name
        cpu_us = statistics.median(times) * 1e6 * samples / 3000
        kernel = timed[f'limit/{name}']
        results['limit'][name] = {
            'kernel': kernel,
            'over_copy': kernel['median_us'] / timed['copy']['median_us'],
            'steps_per_row': samples + 39,
            'tiles_per_row': -(-(samples + 39) // tile),
            'envelope_steps_serial_mean': counts[:, 0].mean().item(),
            'gain_steps_serial_mean': counts[:, 1].mean().item(),
            'gain_steps_serial_max': counts[:, 1].max().item(),
            'tiles_skipped_mean': counts[:, 3].mean().item(),
            'output_peak': out.abs().max().item(),
            'cpu_literal_one_row_us_EXTRAPOLATED': cpu_us,
            'cpu_literal_measured_on_samples': 3000,
            'cpu_row_over_kernel_batch': cpu_us / kernel['median_us']}
        print(json.dumps({name: results['limit'][name]}), flush=True)
    print(json.dumps({k: results[k] for k in (
        'copy', 'shift', 'scale', 'from_audio')}), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
