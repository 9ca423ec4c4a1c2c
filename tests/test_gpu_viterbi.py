"""promonet_amd.viterbi (pm_viterbi) against the CPU oracle of
tests/harmonics_oracle.py, bit for bit: the decode is a pure function of its
fp32 inputs. Log-probabilities are multiples of 1/8 in [-4, 0], so exact ties
are everywhere, and half of the observation is -inf.
"""
import numpy as np
import pytest
import torch

from promonet_amd import viterbi

import harmonics_oracle as oracle
from test_cpu_harmonics import harmonic_transition, interior_transition

pytestmark = pytest.mark.gpu

STATES = [1, 2, 63, 64, 65, 257, 2039]
FRAMES = [1, 2, 3, 37]
KINDS = ['dense', 'harmonic', 'interior']


def eighths(shape, generator):
    return -torch.randint(0, 33, shape, generator=generator) / 8.


def log_transition(kind, states, generator):
    if kind == 'dense':
        return eighths((states, states), generator)
    if kind == 'harmonic':
        return harmonic_transition(states)
    return interior_transition(states)


def observations(batch, frames, states, generator):
    """Half of the entries -inf; row 0 has one frame all -inf; the last row
    of a batch is all -inf from a third of its frames on"""
    x = eighths((batch, frames, states), generator)
    x[torch.rand(batch, frames, states, generator=generator) < .5] = \
        -float('inf')
    x[0, frames // 2] = -float('inf')
    if batch > 1:
        x[-1, frames // 3:] = -float('inf')
    return x


def ragged(batch, frames):
    return [frames, 1, max(1, frames // 2)][:batch]


def want_paths(x, lengths, transition, initial):
    return torch.stack([
        torch.from_numpy(oracle.viterbi(
            x[row].numpy(), transition.numpy(), initial.numpy(),
            lengths[row]))
        for row in range(len(x))])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('states', STATES)
def test_equals_the_oracle(device, states, kind):
    generator = torch.Generator().manual_seed(states * 7 + len(kind))
    transition = log_transition(kind, states, generator)
    initial = eighths((states,), generator)
    if states > 2:
        initial[1] = -float('inf')
    packed = viterbi.Transition(transition.to(device), log_probs=True)
    assert torch.equal(packed.dense().cpu(), transition)
    for frames in FRAMES:
        for batch in (1, 3):
            x = observations(batch, frames, states, generator)
            lengths = ragged(batch, frames)
            want = want_paths(x, lengths, transition, initial)
            got = viterbi.from_probabilities(
                x.to(device), lengths, packed, initial.to(device),
                log_probs=True)
            assert got.dtype == torch.int32 and got.is_cuda
            assert got.shape == (batch, frames)
            assert torch.equal(got.cpu(), want), (frames, batch)
            # a plain tensor is packed on the way in, and full rows need no
            # lengths
            full = viterbi.from_probabilities(
                x.to(device), None, transition.to(device),
                initial.to(device), log_probs=True)
            whole = [frames] * batch
            assert torch.equal(full.cpu(), want if lengths == whole else
                               want_paths(x, whole, transition, initial))
            # a row of the batch equals its own call
            for row in range(batch):
                alone = viterbi.from_probabilities(
                    x[row:row + 1].to(device), lengths[row:row + 1], packed,
                    initial.to(device), log_probs=True)
                assert torch.equal(alone[0], got[row])


@pytest.mark.parametrize('states', [2, 65, 257])
def test_probabilities_are_logged_on_the_way_in(device, states):
    """log_probs=False: the host takes torch.log of the three arguments and
    nothing else. Powers of two keep ties; zero is -inf."""
    generator = torch.Generator().manual_seed(states)
    frames, batch = 37, 3

    def powers(shape):
        p = torch.exp2(-torch.randint(0, 9, shape, generator=generator).float())
        p[torch.rand(shape, generator=generator) < .4] = 0.
        return p

    x, transition, initial = (
        powers((batch, frames, states)), powers((states, states)),
        powers((states,)))
    lengths = ragged(batch, frames)
    got = viterbi.from_probabilities(
        x.to(device), torch.tensor(lengths), transition.to(device),
        initial.to(device))
    logs = [torch.log(item.to(device)).cpu() for item in
            (x, transition, initial)]
    assert torch.equal(got.cpu(), want_paths(logs[0], lengths, *logs[1:]))
    same = viterbi.from_probabilities(
        logs[0].to(device), lengths, logs[1].to(device), logs[2].to(device),
        log_probs=True)
    assert torch.equal(same, got)


@pytest.mark.parametrize('states', [1, 65])
def test_defaults_are_uniform(device, states):
    generator = torch.Generator().manual_seed(states)
    x = observations(3, 37, states, generator).to(device)
    got = viterbi.from_probabilities(x, log_probs=True)
    transition = torch.full((states, states), 1. / states, device=device)
    initial = torch.full((states,), 1. / states, device=device)
    explicit = viterbi.from_probabilities(
        x, None, torch.log(transition), torch.log(initial), log_probs=True)
    assert torch.equal(got, explicit)
    want = want_paths(
        x.cpu(), [37] * 3, torch.log(transition).cpu(),
        torch.log(initial).cpu())
    assert torch.equal(got.cpu(), want)
    probabilities = torch.exp2(-torch.randint(0, 9, (3, 37, states))).float()
    assert torch.equal(
        viterbi.from_probabilities(probabilities.to(device)),
        viterbi.from_probabilities(
            probabilities.to(device), None, transition, initial))


def test_the_band_of_a_tensor_is_packed_once(device):
    transition = eighths((65, 65), torch.Generator().manual_seed(0)).to(device)
    first = viterbi.banded(transition, True)
    assert viterbi.banded(transition, True) is first
    transition[3, 4] = -float('inf')            # a new version: packed again
    second = viterbi.banded(transition, True)
    assert second is not first
    assert torch.equal(second.dense(), transition)


def test_graph_replay_with_other_lengths(device):
    states, frames, batch = 257, 37, 3
    generator = torch.Generator().manual_seed(5)
    transition = harmonic_transition(states)
    initial = eighths((states,), generator)
    packed = viterbi.Transition(transition.to(device), log_probs=True)
    start = initial.to(device)
    x = observations(batch, frames, states, generator)
    static = x.to(device)
    lengths = torch.tensor([37, 1, 18], dtype=torch.int32, device=device)
    viterbi.from_probabilities(static, lengths, packed, start, True)   # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = viterbi.from_probabilities(static, lengths, packed, start, True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(
        out.cpu(), want_paths(x, [37, 1, 18], transition, initial))
    other = observations(batch, frames, states, generator)
    static.copy_(other)
    lengths.copy_(torch.tensor([5, 37, 0], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(
        out.cpu(), want_paths(other, [5, 37, 0], transition, initial))


def test_bad_arguments_raise(device):
    with pytest.raises(ValueError, match='40000 states'):
        viterbi.from_probabilities(
            torch.zeros(1, 1, 40000, device=device), log_probs=True)
    x = torch.zeros(2, 3, 4, device=device)
    with pytest.raises(ValueError):
        viterbi.from_probabilities(x, [3], log_probs=True)
    with pytest.raises(ValueError):
        viterbi.from_probabilities(
            x, None, torch.zeros(5, 5, device=device), log_probs=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        viterbi.from_probabilities(x, None, torch.zeros(4, 4), log_probs=True)
    assert viterbi.from_probabilities(
        torch.zeros(0, 3, 4, device=device)).shape == (0, 3)
