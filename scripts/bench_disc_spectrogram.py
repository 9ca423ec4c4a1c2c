"""The discriminator spectrograms on the device beside the same formulas on
torch's own device ops, in one run (run on the GPU box):

  hip     promonet_amd.model.discriminator, forward, and forward + backward
          (the gradient by the audio under a random upstream gradient);
  torch   the reference's formula on torch device ops (reflect pad,
          torch.stft, norm / abs, permute, log10, clamp, amax, maximum),
          forward, and forward + backward through autograd;
  copy    a device copy moving the bytes the hip path reads and writes, the
          floor of a memory-bound pass. Forward: the audio read and the output
          written per resolution (DB: the output written, read and written
          again). Backward: the audio and the upstream read, the bin gradient
          written and read (8 bytes a bin), the time-domain frames written
          and read, the gradient written (DB: the output and the upstream
          read once more for the sums).

A family is what one discriminator set computes on one audio tensor: R the
three resolutions of DiscriminatorR, CMB the one of DiscriminatorCMB, DB the
six of DiscriminatorMagFree. Shapes: the reference's default BATCH_SIZE x
CHUNK_SIZE (recorded in tests/golden/adversarial.pt) and 256 x 4096. The
three paths are interleaved round by round; device time between events,
median of ROUNDS rounds of CALLS calls after a warm-up of every shape.

Prints one JSON line and writes profiles/disc_spectrogram/bench.json (or
--output).
    python scripts/bench_disc_spectrogram.py
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
from promonet_amd.model import discriminator  # noqa: E402

ROUNDS = 7
FAMILIES = {
    'R': [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)],
    'CMB': [(1024, 256, 1024)],
    'DB': [(n, n // 4, n) for n in (64, 128, 256, 512, 1024, 2048)]}


def hip_one(family, x, sizes):
    if family == 'R':
        return discriminator.spectrogram_resolution(x, sizes)
    if family == 'DB':
        return discriminator.spectrogram_decibel(x, sizes)
    # (the one tensor spectrogram_multiband's bands are views of)
    return discriminator._spectrogram(
        x, promonet_amd._lib.DISC_SPEC_CMB, sizes)[:, None]


def torch_one(family, x, sizes):
    fft_size, hop_size, win_length = sizes
    if family == 'DB':
        X = torch.stft(
            x.squeeze(1), fft_size, hop_size, win_length,
            window=torch.hann_window(win_length).to(x.device),
            return_complex=True).abs()
        x_db = 20. * torch.log10(torch.clamp(X, min=1e-5))
        return torch.max(x_db, x_db.amax() - 80.)
    pad = int((fft_size - hop_size) / 2)
    X = torch.stft(
        torch.nn.functional.pad(x, (pad, pad), mode='reflect').squeeze(1),
        fft_size, hop_size, win_length,
        window=torch.ones(win_length, device=x.device), center=False,
        return_complex=True)
    magnitude = torch.norm(torch.view_as_real(X), p=2, dim=-1).unsqueeze(1)
    if family == 'CMB':
        # (contiguous: the bands' convolutions read it in this order)
        return torch.permute(magnitude, (0, 1, 3, 2)).contiguous()
    return magnitude


def moved_bytes(family, batch, samples):
    forward = backward = 0
    for fft_size, hop_size, _ in FAMILIES[family]:
        pad = fft_size // 2 if family == 'DB' else (fft_size - hop_size) // 2
        frames = 1 + (samples + 2 * pad - fft_size) // hop_size
        elements = batch * (fft_size // 2 + 1) * frames
        audio = batch * samples
        forward += 4 * (audio + elements * (3 if family == 'DB' else 1))
        backward += 4 * (audio + elements + 4 * elements
                         + 2 * batch * frames * fft_size + audio
                         + (2 * elements if family == 'DB' else 0))
    return forward, forward + backward


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
        '--output',
        default=str(ROOT / 'profiles' / 'disc_spectrogram' / 'bench.json'))
    parser.add_argument('--calls', type=int, default=3)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_disc_spectrogram.py needs the GPU')
    device = torch.device('cuda:0')
    golden = torch.load(ROOT / 'tests' / 'golden' / 'adversarial.pt')
    shapes = [(golden['batch_size'], golden['chunk_size']), (256, 4096)]
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'window_size': promonet_amd.WINDOW_SIZE,
               'hopsize': promonet_amd.HOPSIZE, 'cases': {}}
    generator = torch.Generator(device).manual_seed(0)
    for batch, samples in shapes:
        x = (.1 * torch.randn(batch, 1, samples, device=device,
                              generator=generator)).requires_grad_(True)
        for family, resolutions in FAMILIES.items():
            with torch.no_grad():
                upstreams = [torch.randn(
                    hip_one(family, x, sizes).shape, device=device,
                    generator=generator) for sizes in resolutions]

            def forward(one):
                return [one(family, x, sizes) for sizes in resolutions]

            def both(one):
                return torch.autograd.grad(forward(one), x, upstreams)[0]

            copies = {}
            for case, count in zip(('forward', 'forward_backward'),
                                   moved_bytes(family, batch, samples)):
                source = torch.empty(
                    count // 8, dtype=torch.float32, device=device)
                copies[case] = (source, torch.empty_like(source), count)
            with torch.no_grad():
                stages = timed({
                    'hip_forward': lambda: forward(hip_one),
                    'torch_forward': lambda: forward(torch_one),
                    'copy_forward': lambda: copies['forward'][1].copy_(
                        copies['forward'][0])}, args.calls)
            stages.update(timed({
                'hip_forward_backward': lambda: both(hip_one),
                'torch_forward_backward': lambda: both(torch_one),
                'copy_forward_backward':
                    lambda: copies['forward_backward'][1].copy_(
                        copies['forward_backward'][0])}, args.calls))
            stages['bytes_forward'] = copies['forward'][2]
            stages['bytes_forward_backward'] = copies['forward_backward'][2]
            del copies
            stages['resolutions'] = [list(r) for r in resolutions]
            ours, theirs = both(hip_one), both(torch_one)
            stages['gradient_relative_l2'] = (
                (ours - theirs).norm() / theirs.norm()).item()
            with torch.no_grad():
                stages['output_max_abs_difference'] = max(
                    (a.reshape(b.shape) - b).abs().max().item()
                    for a, b in zip(forward(hip_one), forward(torch_one)))
            results['cases'][f'{family}, {batch} x {samples}'] = stages
            del upstreams, ours, theirs
            torch.cuda.empty_cache()
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
