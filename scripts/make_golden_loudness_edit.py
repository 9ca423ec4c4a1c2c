"""Write tests/golden/loudness_edit.pt from the real reference (build host
only).

Imports the reference with oracle/reference_import.py as it is and runs its
own `promonet.preprocess.loudness.limit` and `shift` on seeded inputs. Asserts
that the restatement (tests/loudness_edit_oracle.py) equals them, `limit` bit
for bit and `shift` within 1e-12 in float64, and stores tensors only: the
inputs, the parameters and the reference's outputs. `scale` needs librosa's
A-weighting, which is absent here, and gets no golden.

    python scripts/make_golden_loudness_edit.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

# (delay, attack_coef, release_coef, threshold)
LIMIT_CASES = ((40, .9, .9995, .99), (7, .5, .99, .5), (1, .9, .9995, .99))
SHIFT_CASES = ((9, 2321), (2, 513), (40, 1000))     # (frames, samples)


def limiter_input():
    """1 600 samples: quiet, a burst, a spike, near silence, a tail"""
    gen = torch.Generator().manual_seed(114141)
    x = torch.randn(1600, generator=gen) * .25
    x[200:220] *= 8
    x[700] = 3.
    x[900:1300] *= .01
    return x[None]


def main():
    import reference_import
    import loudness_edit_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    reference = promonet.preprocess.loudness
    out = {}
    audio = limiter_input()
    out['limit/audio'] = audio
    for index, case in enumerate(LIMIT_CASES):
        delay, attack, release, threshold = case
        want = reference.limit(audio.clone(), delay, attack, release,
                               threshold)
        got, _ = oracle.limit_literal(audio, delay, attack, release,
                                      threshold)
        assert want.dtype == torch.float32 and want.shape == audio.shape
        assert torch.equal(got, want), case
        assert not torch.equal(want, audio), case
        out[f'limit/case{index}/parameters'] = torch.tensor(
            case, dtype=torch.float64)
        out[f'limit/case{index}/output'] = want
    worst = 0.
    for index, (frames, samples) in enumerate(SHIFT_CASES):
        x, value = oracle.shift_inputs(frames, samples)
        want = reference.shift(x.double(), value.double())
        got = oracle.shift64(x, value)
        error = ((got - want).abs() / want.abs()).max().item()
        worst = max(worst, error)
        assert want.dtype == torch.float64 and error <= 1e-12, error
        out[f'shift/case{index}/shape'] = torch.tensor([frames, samples])
        out[f'shift/case{index}/audio'] = x
        out[f'shift/case{index}/value'] = value
        out[f'shift/case{index}/output'] = want
    x, _ = oracle.shift_inputs(1, 300)
    want = reference.shift(x.double(), -6.5)
    assert torch.equal(oracle.shift64(x, -6.5), want)
    out['shift/scalar/audio'] = x
    out['shift/scalar/value'] = torch.tensor(-6.5, dtype=torch.float64)
    out['shift/scalar/output'] = want
    assert all(isinstance(v, torch.Tensor) for v in out.values())
    path = ROOT / 'tests' / 'golden' / 'loudness_edit.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 200 * 1024, size
    print(f'{path}: {size} bytes, shift restatement relative error '
          f'{worst:.3e}')


if __name__ == '__main__':
    main()
