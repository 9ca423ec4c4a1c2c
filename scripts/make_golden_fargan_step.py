"""Write tests/golden/fargan_step.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py under config/fargan.py,
loads oracle.random_state_fargan(SEED) into its Generator and runs
`FARGAN.step` frame by frame on the CPU in two cases:

  warm    zero state, WARM frames, then RUN more frames from the state and
          previous samples the warm-up ended in;
  random  RUN frames from a random state: GRU states U(-1, 1), a sub-frame
          input of tanh-range features and samples of the history, and
          random previous samples.

Asserts that tests/fargan_step_oracle.py (the restatement, from an arbitrary
state) equals the reference, then stores the seed, the inputs, the initial
and final states, the previous samples and the audio - tensors only; the seed
rebuilds the weights.

    python scripts/make_golden_fargan_step.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

SEED = 0          # the weights of tests/golden/generator_fargan.pt
WARM, RUN = 5, 8


def main():
    import reference_import
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load(
        [reference_import.REFERENCE_ROOT / 'config' / 'fargan.py'])
    import restatement as oracle
    import fargan_step_oracle
    assert promonet.MODEL == 'fargan'
    torch.manual_seed(0)
    generator = promonet.model.Generator().eval()
    state = oracle.random_state_fargan(seed=SEED)
    state['pitch_distribution'] = \
        generator.state_dict()['pitch_distribution'].clone()
    generator.load_state_dict(state)
    model = generator.model
    weights = oracle.fargan_weights(state)
    fargan = promonet.model.fargan

    def reference(features, g, previous, states):
        frames = []
        with torch.inference_mode():
            for frame in features.permute(2, 0, 1):
                out, previous, states = model.step(frame, g, previous, states)
                frames.append(out)
        return torch.cat(frames, dim=1)[:, None], previous, tuple(states)

    def pinned(name, features, g, previous, states):
        audio, previous_out, states_out = reference(
            features, g, previous, states)
        with torch.inference_mode():
            mine = fargan_step_oracle.fargan_stream(
                weights, features, g, previous, states)
        error = max((a - b).abs().max().item() for a, b in zip(
            (audio, previous_out) + states_out, mine[:2] + tuple(mine[2])))
        print(f'fargan step {name}: restatement vs reference {error:.3e}')
        assert error <= 1e-6, (name, error)
        return audio, previous_out, states_out

    out = {'seed': torch.tensor(SEED), 'warm_frames': torch.tensor(WARM)}
    gen = torch.Generator().manual_seed(7)

    # (a) warm-up from zero state, then a chunk from the state it left
    features, g = fargan_step_oracle.features(2, WARM + RUN, state, seed=41)
    zero = fargan.initialize_recurrent_state(2, 'cpu')
    assert [tuple(t.shape) for t in zero] == [(2, 256)] * 3 + [(2, 260)]
    _, previous, states = pinned(
        'warm-up', features[..., :WARM], g, torch.zeros(2, 1, 512), zero)
    audio, previous_out, states_out = pinned(
        'warm', features[..., WARM:], g, previous, states)
    out['warm/features'] = features
    out['warm/global'] = g
    out['warm/previous'] = previous
    out['warm/states'] = torch.cat(states, dim=1)
    out['warm/audio'] = audio
    out['warm/previous_out'] = previous_out
    out['warm/states_out'] = torch.cat(states_out, dim=1)

    # (b) a random state
    batch = 3
    features, g = fargan_step_oracle.features(batch, RUN, state, seed=42)
    previous = (torch.rand(batch, 1, 512, generator=gen) * .4 - .2)
    lookback = previous[:, 0, 512 - 200:512 - 200 + 68]
    states = tuple(
        torch.rand(batch, 256, generator=gen) * 2. - 1. for _ in range(3)) + (
        torch.cat((torch.rand(batch, 128, generator=gen) * 1.8 - .9,
                   previous[:, 0, -128:-64], lookback), dim=1),)
    audio, previous_out, states_out = pinned(
        'random', features, g, previous, states)
    out['random/features'] = features
    out['random/global'] = g
    out['random/previous'] = previous
    out['random/states'] = torch.cat(states, dim=1)
    out['random/audio'] = audio
    out['random/previous_out'] = previous_out
    out['random/states_out'] = torch.cat(states_out, dim=1)

    out = {k: v.detach().clone().contiguous() for k, v in out.items()}
    path = ROOT / 'tests' / 'golden' / 'fargan_step.pt'
    torch.save(out, path)
    print(f'wrote {path} ({path.stat().st_size} bytes)')


if __name__ == '__main__':
    main()
