"""Digest of what every entry on the Stockham STFT (pm_stockham.h) computes.

For the spectral-convergence loss (pm_sc_stft, pm_sc_forward, pm_sc_adjoint),
the signal loss and the discriminator spectrograms (pm_disc_spec_forward,
pm_disc_spec_backward), on seeded inputs generated on the CPU: one line per
output tensor with its sha256. The kernels use no float atomics, so two builds
of the same arithmetic give the same lines, and a change that claims to leave
the arithmetic alone shows it by equal listings from the two libraries, each
in a process of its own. Hashes only; needs a GPU. The shapes are the smallest
that reach every radix, a partial last workgroup of a row, one frame a
workgroup, both reflect margins folding onto the same samples, and a hop that
does not divide the frame.

    PROMONET_HIP_LIB=<build>/libpromonet_hip.so python scripts/stft_bits.py
"""
import hashlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from promonet_amd import _lib, loss                         # noqa: E402
from promonet_amd.model import discriminator                # noqa: E402

# (fft_size, hop_size, samples, batch)
LOSS = [(64, 16, 1000, 2), (80, 20, 1000, 2), (2560, 640, 1300, 3),
        (1024, 120, 4096, 2)]
SIGNAL = (3, 1000)
# (mode, (n_fft, hop_length, win_length), samples); batch 2
DISC = [('R', (512, 50, 240), 232), ('R', (1024, 120, 600), 4096),
        ('CMB', (1024, 256, 1024), 4096), ('DB', (64, 16, 64), 1000),
        ('DB', (2048, 512, 2048), 1025)]
DEVICE = torch.device('cuda', 0)
GENERATOR = torch.Generator().manual_seed(20)


def noise(*shape):
    return (.1 * torch.randn(*shape, generator=GENERATOR)).to(DEVICE)


def show(name, tensor):
    data = tensor.detach().cpu().contiguous().numpy().tobytes()
    print(f'{name:52} {hashlib.sha256(data).hexdigest()}')


def loss_lines(fft_size, hop_size, samples, batch):
    name = f'sc {fft_size}/{hop_size} {batch}x{samples}'
    x, y = noise(batch, samples), noise(batch, samples)
    window = loss._named_window(DEVICE, 'hann_window', fft_size, fft_size)
    twiddle = loss._twiddle(DEVICE, fft_size)
    s, _ = loss._stft_call(x, window, twiddle, fft_size, hop_size)
    show(f'{name} stft s', s)
    _, gradient = loss._stft_call(
        x, window, twiddle, fft_size, hop_size, upstream=noise(*s.shape),
        want_s=False, want_gradient=True)
    show(f'{name} stft G', gradient)
    sums, workspace = loss._forward_call(
        x, y, window, twiddle, fft_size, hop_size, True)
    show(f'{name} forward sums', sums)
    show(f'{name} forward G', workspace[:4 * gradient.numel()])
    scale, start = noise(1), noise(batch, samples)
    for accumulate in (False, True):
        grad_x = start.clone()
        loss._adjoint_call(workspace, window, twiddle, scale, grad_x,
                           fft_size, hop_size, accumulate)
        show(f'{name} adjoint accumulate {int(accumulate)}', grad_x)


def signal_lines(rows, samples):
    y_true = noise(rows, samples)
    y_pred = noise(rows, samples).requires_grad_()
    value = loss.signal(y_true, y_pred)
    show(f'signal {rows}x{samples} value', value)
    value.backward(noise(1)[0])
    show(f'signal {rows}x{samples} gradient', y_pred.grad)


def disc_lines(mode, resolution, samples):
    name = f'{mode} {"/".join(map(str, resolution))} 2x{samples}'
    x = noise(2, samples)
    sizes = discriminator._sizes(
        getattr(_lib, f'DISC_SPEC_{mode}'), resolution, samples)
    window, twiddle = discriminator._tables(DEVICE, sizes)
    out, stats = discriminator._forward_call(x, window, twiddle, sizes)
    show(f'{name} forward', out)
    if stats is not None:
        show(f'{name} forward stats', stats)
    upstream, scale, start = noise(*out.shape), noise(1), noise(2, samples)
    saved = () if stats is None else (out, stats)
    for into in (None, start):
        for factor in (None, scale):
            grad_x = discriminator._backward_call(
                x, window, twiddle, sizes, upstream, *saved,
                into=None if into is None else into.clone(), scale=factor)
            show(f'{name} backward accumulate {int(into is not None)} '
                 f'scale {int(factor is not None)}', grad_x)


def main():
    for case in LOSS:
        loss_lines(*case)
    signal_lines(*SIGNAL)
    for case in DISC:
        disc_lines(*case)


if __name__ == '__main__':
    main()
