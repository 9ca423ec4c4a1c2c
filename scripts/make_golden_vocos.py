"""Write tests/golden/vocos.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py under
config/baselines/vocos.py, builds its MelGenerator, loads
tests/vocos_oracle.py::random_state_vocos(seed) into it and runs
`model.model(mels, g)` (Vocos itself: the reference's linear_to_mel needs
librosa) and `prepare_global_features` on a few shapes. Asserts that the
restatement equals the reference, then stores the seed, the inputs, the
outputs, the state-dict shapes and the constants - tensors only, no weights:
the seed rebuilds them at the full 512 / 1536 width.

    python scripts/make_golden_vocos.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

SEED = 11
SHAPES = ((1, 1), (2, 7), (3, 40), (1, 17))      # (batch, frames)


def main():
    import reference_import
    import vocos_oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    config = reference_import.REFERENCE_ROOT / 'config' / 'baselines' / \
        'vocos.py'
    promonet = reference_import.load([config])
    assert promonet.MODEL == 'vocos' and promonet.NUM_FEATURES == 80
    torch.manual_seed(0)
    generator = promonet.model.MelGenerator()
    reference_state = generator.state_dict()
    state = vocos_oracle.random_state_vocos(SEED)
    speaker_table = torch.randn(
        promonet.NUM_SPEAKERS, promonet.SPEAKER_CHANNELS,
        generator=torch.Generator().manual_seed(SEED + 1))
    full = {'model.' + k: v for k, v in state.items()}
    full['speaker_embedding.weight'] = speaker_table
    full['default_previous_samples'] = reference_state[
        'default_previous_samples']
    generator.load_state_dict(full)
    generator.eval()

    out = {'seed': torch.tensor(SEED),
           'num_entries': torch.tensor(len(reference_state)),
           'num_elements': torch.tensor(
               sum(v.numel() for v in reference_state.values())),
           'constants': torch.tensor([
               promonet.NUM_FEATURES, promonet.GLOBAL_CHANNELS,
               promonet.VOCOS_CHANNELS, promonet.VOCOS_POINTWISE_CHANNELS,
               promonet.VOCOS_LAYERS, promonet.NUM_FFT, promonet.HOPSIZE])}
    for key, value in reference_state.items():
        out['shape/' + key] = torch.tensor(list(value.shape))
    gen = torch.Generator().manual_seed(SEED + 2)
    worst = 0.
    for index, (batch, frames) in enumerate(SHAPES):
        mels = torch.randn(batch, 80, frames, generator=gen) - 4.
        speakers = torch.randint(0, promonet.NUM_SPEAKERS, (batch,),
                                 generator=gen)
        ones = torch.ones(batch)
        with torch.no_grad():
            g = generator.prepare_global_features(speakers, ones, ones)
            want = generator.model(mels, g)
        got = vocos_oracle.vocos(
            mels, vocos_oracle.global_features(speakers, speaker_table), state)
        error = (got - want).abs().max().item()
        worst = max(worst, error)
        assert want.shape == (batch, 1, frames * 256), want.shape
        assert error <= 1e-6, (batch, frames, error)
        out[f'case{index}/mels'] = mels
        out[f'case{index}/speakers'] = speakers
        out[f'case{index}/audio'] = want
    out['speaker_table_seed'] = torch.tensor(SEED + 1)
    path = ROOT / 'tests' / 'golden' / 'vocos.pt'
    torch.save(out, path)
    print(f'{path}: {path.stat().st_size} bytes, restatement max-abs '
          f'{worst:.3e}')


if __name__ == '__main__':
    main()
