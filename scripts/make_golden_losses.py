"""Write tests/golden/losses.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py under config/fargan.py
(MEL_LOSS = False, SPECTRAL_CONVERGENCE_LOSS = True) and runs
`promonet.loss.stft`, `SpectralConvergence`, `MultiResolutionSpectralConvergence`
(with backward) and `signal` on the seeded inputs of
tests/losses_oracle.py::inputs, in float64: the modules' windows are replaced
by the same torch window function at float64, so that the golden is the
reference's arithmetic at the yardstick's precision. Asserts that the
restatement (tests/losses_oracle.py) equals all of it within 1e-6 relative and
stores tensors only: seeds, shapes, losses, gradients (as fp32) and one
transform.

    python scripts/make_golden_losses.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

CASES = ((0, 2, 4096), (1, 1, 1281))            # (seed, batch, samples)
SINGLE = (1024, 120, 600)                       # SpectralConvergence defaults


def relative(got, want):
    return ((got - want).abs().max() / want.abs().max()).item()


def double_windows(module):
    for loss in getattr(module, 'stft_losses', [module]):
        loss.window = torch.hann_window(loss.win_length, dtype=torch.float64)
    return module


def main():
    import reference_import
    import losses_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    config = reference_import.REFERENCE_ROOT / 'config' / 'fargan.py'
    promonet = reference_import.load([config])
    assert promonet.SPECTRAL_CONVERGENCE_LOSS and not promonet.MEL_LOSS
    out, worst = {}, 0.
    for index, (seed, batch, samples) in enumerate(CASES):
        x, y = (t.double() for t in oracle.inputs(seed, batch, samples))
        key = f'case{index}/'
        out[key + 'seed'] = torch.tensor(seed)
        out[key + 'shape'] = torch.tensor([batch, samples])
        errors = []

        # stft at the largest and the smallest default resolution
        for fft_size in (2560, 80):
            window = torch.hann_window(fft_size, dtype=torch.float64)
            want = promonet.loss.stft(x, fft_size, fft_size // 4, fft_size,
                                      window)
            got = oracle.stft(x, fft_size, fft_size // 4, fft_size)
            errors.append(relative(got, want))
            if fft_size == 2560:
                out[key + 'stft2560'] = want.float()

        # each default resolution, and the module's own defaults
        losses = []
        for sizes in oracle.DEFAULT_RESOLUTIONS + (SINGLE,):
            module = double_windows(
                promonet.loss.SpectralConvergence('cpu', *sizes))
            want = module(x[:, None], y[:, None])
            errors.append(relative(
                oracle.spectral_convergence(x, y, *sizes), want))
            losses.append(want)
        out[key + 'resolution_losses'] = torch.stack(losses[:-1])
        out[key + 'single_loss'] = losses[-1]

        # the multi-resolution loss and its gradient
        module = double_windows(
            promonet.loss.MultiResolutionSpectralConvergence('cpu'))
        leaf = x[:, None].clone().requires_grad_(True)
        want = module(leaf, y[:, None])
        want.backward()
        mine = x.clone().requires_grad_(True)
        got = oracle.multi_resolution(mine, y)
        got.backward()
        errors.append(relative(got.detach(), want.detach()))
        errors.append(relative(mine.grad, leaf.grad[:, 0]))
        out[key + 'loss'] = want.detach()
        out[key + 'gradient'] = leaf.grad[:, 0].float()

        # signal(y_true, y_pred) and its gradient by y_pred
        leaf = x.clone().requires_grad_(True)
        want = promonet.loss.signal(y, leaf)
        want.backward()
        errors.append(relative(oracle.signal(y, x), want.detach()))
        errors.append(relative(oracle.signal_gradient(y, x), leaf.grad))
        out[key + 'signal'] = want.detach()
        out[key + 'signal_gradient'] = leaf.grad.float()

        assert max(errors) <= 1e-6, (index, errors)
        worst = max(worst, max(errors))
    assert all(isinstance(v, torch.Tensor) for v in out.values())
    path = ROOT / 'tests' / 'golden' / 'losses.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 200 * 1024, size
    print(f'{path}: {size} bytes, restatement relative error {worst:.3e}')


if __name__ == '__main__':
    main()
