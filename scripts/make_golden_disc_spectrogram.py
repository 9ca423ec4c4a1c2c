"""Write tests/golden/disc_spectrogram.pt from the real reference (build host
only).

Imports the reference with oracle/reference_import.py and runs its own
`DiscriminatorR.spectrogram`, `DiscriminatorCMB.spectrogram` and
`SpecDiscriminatorBase.spectrogram` (promonet/model/discriminator.py) in
float64 on the small inputs of tests/disc_spectrogram_oracle.py, with the
gradient of <upstream, output> by autograd, and asserts that the float64
restatement equals them to 1e-12 relative (of the largest value of the
tensor).

`torchaudio` is not on this machine and reference_import mocks it: for DB the
script puts the oracle's restatement of `amplitude_to_DB` (the published
formula) into the reference's module, so the STFT half of that method is
pinned and the decibel half is unpinned.

The file stays under 200 KB: the inputs are the oracle's seeded ones (the
first eight samples of each are kept, to catch a generator that changed), and
of every output and gradient every OUTPUT_STRIDE-th and GRADIENT_STRIDE-th
element of the flattened tensor is kept, in float64.

    python scripts/make_golden_disc_spectrogram.py
"""
import sys
import types
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

OUTPUT_STRIDE, GRADIENT_STRIDE = 7, 3


def reference_output(promonet, kind, x, sizes):
    """The reference's method on x (B, 1, T) float64, as one tensor"""
    model = promonet.model.discriminator
    if kind == 'R':
        return model.DiscriminatorR.spectrogram(
            types.SimpleNamespace(resolution=sizes), x)
    if kind == 'CMB':
        discriminator = model.DiscriminatorCMB()
        assert discriminator.window_length == sizes[0]
        assert discriminator.hop_size == sizes[1]
        return torch.cat(discriminator.spectrogram(x), -1), discriminator.bands
    return model.SpecDiscriminatorBase.spectrogram(
        types.SimpleNamespace(resolution=list(sizes)), x)


def main():
    import reference_import
    import disc_spectrogram_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    model = promonet.model.discriminator
    model.torchaudio.functional.amplitude_to_DB = oracle.amplitude_to_db

    def close(got, want):
        scale = want.abs().max()
        assert (got - want).abs().max() <= 1e-12 * scale, (
            (got - want).abs().max(), scale)

    out = {'output_stride': OUTPUT_STRIDE, 'gradient_stride': GRADIENT_STRIDE}
    for name, (kind, sizes, samples) in oracle.CASES.items():
        want = oracle.truth(name)
        leaf = want['x'].double()[:, None].clone().requires_grad_(True)
        result = reference_output(promonet, kind, leaf, sizes)
        if kind == 'CMB':
            result, bands = result
            assert [tuple(b) for b in bands] == list(oracle.DEFAULT_EDGES)
            out['edges'] = [list(b) for b in bands]
        assert result.dtype == torch.float64
        assert result.shape == want['out'].shape, (name, result.shape)
        frames = result.shape[2 if kind == 'CMB' else -1]
        assert frames == oracle.FRAMES[name], (name, frames)
        result.backward(want['upstream'].double())
        close(want['out'], result.detach())
        close(want['gradient'], leaf.grad[:, 0])
        out[name] = {
            'head': want['x'][:, :8].clone(),
            'shape': list(result.shape),
            'out': result.detach().flatten()[::OUTPUT_STRIDE].clone(),
            'gradient': leaf.grad.flatten()[::GRADIENT_STRIDE].clone()}
        print(f'{name}: {tuple(result.shape)}, {frames} frames: the oracle '
              'equals the reference')
    path = ROOT / 'tests' / 'golden' / 'disc_spectrogram.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 200 * 1024, size
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
