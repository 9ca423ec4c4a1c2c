"""The multi-resolution spectral-convergence loss on the device beside the
same formula on torch's own device ops, in one run (run on the GPU box):

  hip     promonet_amd.loss.MultiResolutionSpectralConvergence, forward, and
          forward + backward;
  torch   sqrt(clamp(|torch.stft|, 1e-7)) per resolution (hipFFT) and the
          same reductions, forward, and forward + backward through autograd;
  copy    a device copy of the bytes the hip path moves (x and y read per
          resolution; with the backward also G written and read, the frames
          written and read, grad_x read and written), the floor of a
          memory-bound pass.

on 256 x 4096 (the reference's training batch) and 32 x 4096. The three are
interleaved round by round; device time between events, median of ROUNDS
rounds of CALLS calls after a warm-up of every shape. Also reports the
largest difference between the two losses and gradients.

Prints one JSON line and writes profiles/losses/bench.json (or --output).
    python scripts/bench_losses.py
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import promonet_amd  # noqa: E402

ROUNDS = 7
RESOLUTIONS = tuple((n, n // 4, n) for n in (2560, 1280, 640, 320, 160, 80))


def torch_loss(x, y, windows):
    total = 0.
    for (fft_size, hop_size, win_length), window in zip(RESOLUTIONS, windows):
        def s(audio):
            return torch.sqrt(torch.clamp(torch.stft(
                audio, fft_size, hop_size, win_length, window,
                return_complex=True).abs(), min=1e-7))
        s_x, s_y = s(x), s(y)
        total = total + (s_y - s_x).abs().sum() / s_y.sum()
    return total / len(RESOLUTIONS)


def moved_bytes(batch, samples, backward):
    """What the hip path reads and writes, from the shapes"""
    total = 0
    for fft_size, hop_size, _ in RESOLUTIONS:
        frames, bins = 1 + samples // hop_size, fft_size // 2 + 1
        total += 2 * batch * samples * 4
        if backward:
            total += 2 * batch * bins * frames * 8      # G written, read
            total += 2 * batch * frames * fft_size * 4  # frames written, read
            total += 2 * batch * samples * 4            # grad_x read, written
    return total


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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'losses' / 'bench.json'))
    parser.add_argument('--batches', type=int, nargs='+', default=[256, 32])
    parser.add_argument('--samples', type=int, default=4096)
    parser.add_argument('--calls', type=int, default=20)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_losses.py needs the GPU')
    device = torch.device('cuda:0')
    module = promonet_amd.loss.MultiResolutionSpectralConvergence(device)
    windows = [torch.hann_window(r[2], device=device) for r in RESOLUTIONS]
    results = {'device': torch.cuda.get_device_name(0),
               'samples': args.samples, 'rounds': ROUNDS, 'shapes': {}}
    for batch in args.batches:
        generator = torch.Generator().manual_seed(batch)
        x = (.1 * torch.randn(batch, args.samples, generator=generator)).to(
            device)
        y = (.1 * torch.randn(batch, args.samples, generator=generator)).to(
            device)
        leaf = x.clone().requires_grad_(True)

        def hip_both():
            return torch.autograd.grad(module(leaf, y), leaf)[0]

        def torch_both():
            return torch.autograd.grad(torch_loss(leaf, y, windows), leaf)[0]

        copies = {}
        for name, backward in (('forward', False), ('both', True)):
            count = moved_bytes(batch, args.samples, backward) // 8
            source = torch.empty(count, dtype=torch.float32, device=device)
            copies[name] = (source, torch.empty_like(source))
        stages = timed({
            'hip_forward': lambda: module(x, y),
            'torch_forward': lambda: torch_loss(x, y, windows),
            'copy_forward': lambda: copies['forward'][1].copy_(
                copies['forward'][0]),
            'hip_forward_backward': hip_both,
            'torch_forward_backward': torch_both,
            'copy_forward_backward': lambda: copies['both'][1].copy_(
                copies['both'][0])}, args.calls)
        stages['bytes_forward'] = moved_bytes(batch, args.samples, False)
        stages['bytes_forward_backward'] = moved_bytes(
            batch, args.samples, True)
        with torch.no_grad():
            ours, theirs = module(x, y), torch_loss(x, y, windows)
        stages['loss_hip'], stages['loss_torch'] = ours.item(), theirs.item()
        ours, theirs = hip_both(), torch_both()
        stages['gradient_relative_l2'] = (
            (ours - theirs).norm() / theirs.norm()).item()
        results['shapes'][f'{batch} x {args.samples}'] = stages
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
