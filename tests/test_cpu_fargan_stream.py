"""FARGAN streaming API on the host: the reference's `step` signature and
state shapes, and the step restatement behind the streaming golden."""
import inspect
from pathlib import Path

import pytest
import torch

import fargan_step_oracle
import restatement as oracle

GOLDEN = Path(__file__).resolve().parent / 'golden'


def test_initialize_recurrent_state_has_the_reference_shapes():
    """fargan.py:406-415: (B, 256) x 3 and (B, 4 * 64 + 4), fp32."""
    from promonet_amd.model import initialize_recurrent_state
    from promonet_amd.model.fargan import initialize_recurrent_state as same
    assert same is initialize_recurrent_state
    states = initialize_recurrent_state(3, 'cpu')
    assert isinstance(states, tuple) and len(states) == 4
    assert [tuple(t.shape) for t in states] == [(3, 256)] * 3 + [(3, 260)]
    assert all(t.dtype == torch.float32 and not t.any() for t in states)
    # the restatement's states (what the reference's step returns) agree
    state = oracle.random_state_fargan(seed=0)
    features = torch.zeros(1, 114, 1)
    features[:, -1] = 100.
    _, returned, _ = oracle.fargan_forward(
        features, torch.zeros(1, 258, 1), torch.zeros(1, 1, 512), state,
        return_states=True)
    assert [tuple(t.shape) for t in returned] == [(1, 256)] * 3 + [(1, 260)]


def test_step_signature_matches_the_reference():
    """FARGAN.step(features, global_features, previous_samples, states)
    (fargan.py:65-71); stream() is the chunked form."""
    from promonet_amd.model import FARGAN
    names = list(inspect.signature(FARGAN.step).parameters)
    assert names == [
        'self', 'features', 'global_features', 'previous_samples', 'states']
    stream = inspect.signature(FARGAN.stream).parameters
    assert list(stream)[:5] == names
    assert stream['previous_samples'].default is None
    assert stream['states'].default is None


def test_step_rejects_host_tensors():
    from promonet_amd.model import FARGAN, initialize_recurrent_state
    model = FARGAN(113, 258)
    with pytest.raises(RuntimeError):
        model.step(torch.zeros(1, 114), torch.zeros(1, 258),
                   torch.zeros(1, 1, 512), initialize_recurrent_state(1, 'cpu'))
    with pytest.raises(RuntimeError):
        model.stream(torch.zeros(1, 114, 2), torch.zeros(1, 258))


def test_step_restatement_reproduces_the_golden():
    """The golden's audio and states (written by the reference's step) from
    the restatement, and the zero-state chunk equals fargan_forward."""
    golden = torch.load(GOLDEN / 'fargan_step.pt', weights_only=False)
    state = oracle.random_state_fargan(seed=int(golden['seed']))
    weights = oracle.fargan_weights(state)
    warm = int(golden['warm_frames'])
    for case in ('warm', 'random'):
        states = golden[f'{case}/states'].split((256, 256, 256, 260), dim=1)
        features = golden[f'{case}/features']
        if case == 'warm':
            features = features[..., warm:]
        with torch.inference_mode():
            audio, previous, states = fargan_step_oracle.fargan_stream(
                weights, features, golden[f'{case}/global'],
                golden[f'{case}/previous'], states)
        assert (audio - golden[f'{case}/audio']).abs().max() < 1e-6
        assert (previous - golden[f'{case}/previous_out']).abs().max() < 1e-6
        assert (torch.cat(states, 1) -
                golden[f'{case}/states_out']).abs().max() < 1e-6
    features = golden['warm/features'][..., :warm]
    g = golden['warm/global']
    with torch.inference_mode():
        want, want_states, want_previous = oracle.fargan_forward(
            features, g[..., None], torch.zeros(2, 1, 512), state,
            return_states=True)
        got, previous, states = fargan_step_oracle.fargan_stream(
            weights, features, g, torch.zeros(2, 1, 512),
            tuple(torch.zeros(2, n) for n in (256, 256, 256, 260)))
    assert torch.equal(got, want) and torch.equal(previous[:, 0], want_previous)
    assert torch.equal(torch.cat(states, 1), torch.cat(want_states, 1))
    assert (torch.cat(states, 1) - golden['warm/states']).abs().max() < 1e-6
