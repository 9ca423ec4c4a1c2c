"""FARGAN on the GPU where a trained network lives, and with the storage
rounding taken out of the comparison.

test_gpu_fargan.py / test_gpu_fargan_stream.py run randomly initialised
weights from zero state (gate pre-activations below .4, GRU states below
.2), and their f16 / 'mixed' gates have to absorb the rounding of the stored
weights. Here (tests/fargan_probe.py, its footing in
test_cpu_fargan_probe.py):

- one teacher-forced frame (`step`, 4 dependent sub-frame steps) from O(1)
  states and previous samples at the pitch-period edges, with GRU and gate
  weights x 6 - saturated activations, GRU updates with z at 0 and 1 - and
  with units pushed past the overflow ends of fg_tanh / fg_sigmoid; the
  returned states expose every hidden unit unattenuated;
- the reference is the float64 oracle on the weights THE ENGINE computes
  with: folded on the device by the engine's own fold kernel, then rounded
  to f16 where the storage type stores f16. What is left is fp32 arithmetic
  in another summation order, so the f16 and 'mixed' gates are the fp32
  gates.

Gates (fargan_probe.GATES, FORWARD_GATES, STREAM_GATES): <= 3x what MI355X
measures, recorded beside them; test_cpu_fargan_probe.py::test_sensitivity holds them below the
effect of every planted defect."""
import pytest
import torch

import fargan_probe as probe
import fargan_step_oracle
from util import check, max_abs, to_cl

pytestmark = pytest.mark.gpu

DTYPES = ('fp32', 'mixed', 'f16')
STATES = ('gru1', 'gru2', 'gru3', 'subframe_input')


@pytest.fixture(scope='module')
def world(device):
    """The weight sets, the case table, and per (set, dtype): the model and
    the state the engine computes with (device fold, storage rounding)."""
    import promonet_amd
    from promonet_amd import _lib

    def fold(g, v):
        g, v = g.to(device).contiguous(), v.to(device).contiguous()
        out = torch.empty_like(v)
        _lib.check(_lib.lib().pm_fold_weight_norm(
            _lib.ptr(g), _lib.ptr(v), _lib.ptr(out), v.shape[0], v.shape[1],
            _lib.stream()))
        torch.cuda.synchronize()
        return out.cpu()

    base = probe.base_state()
    sets = {name: make(base) for name, make in probe.WEIGHT_SETS.items()}

    class World:
        table = probe.cases(state=base)
        states = sets
        folded = {name: probe.folded_state(state, fold)
                  for name, state in sets.items()}
        models, oracles = {}, {}

        def model(self, name, dtype, mode):
            if (name, dtype) not in self.models:
                model = promonet_amd.model.FARGAN(113, 258)
                model.load_state_dict({
                    k[len('model.'):]: v for k, v in self.states[name].items()
                    if k.startswith('model.')})
                model.weight_dtype = dtype
                self.models[name, dtype] = model.to(device).eval()
            self.models[name, dtype].kernel_mode = mode
            return self.models[name, dtype]

        def rounded(self, name, dtype):
            return probe.rounded_state(self.folded[name], dtype)

        def oracle(self, name, dtype, batch):
            """float64 oracle of the teacher-forced frame, computed once"""
            if (name, dtype, batch) not in self.oracles:
                self.oracles[name, dtype, batch] = probe.run_oracle(
                    self.rounded(name, dtype), self.table[batch])
            return self.oracles[name, dtype, batch]

        def step(self, model, batch, rows=None):
            features, g, previous, states = self.table[batch]
            if rows is not None:
                features, g, previous = features[rows], g[rows], previous[rows]
                states = tuple(s[rows] for s in states)
            with torch.inference_mode():
                return model.step(
                    features.to(device), g.to(device), previous.to(device),
                    tuple(s.to(device) for s in states))
    return World()


@pytest.mark.parametrize('name', list(probe.WEIGHT_SETS))
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_teacher_forced_step(world, dtype, mode, name):
    """One frame from given states, batches of 3, 37 and 70 (one, two and
    four utterances in lockstep per cluster, with padded slots): audio,
    previous samples and each of the four states against the float64 oracle
    on the engine's own rounded weights."""
    model = world.model(name, dtype, mode)
    for batch in probe.BATCHES:
        audio, previous, states = world.step(model, batch)
        want_audio, want_previous, want_states = world.oracle(
            name, dtype, batch)
        assert audio.shape == (batch, 256) and previous.shape == (batch, 1, 512)
        assert [tuple(s.shape) for s in states] == [
            (batch, n) for n in probe.STATE_SIZES]
        assert torch.isfinite(audio).all() and torch.isfinite(previous).all()
        assert all(torch.isfinite(s).all() for s in states)
        errors = {'audio': max_abs(audio, want_audio),
                  'previous': max_abs(previous, want_previous)}
        for label, got, want in zip(STATES, states, want_states):
            errors[label] = max_abs(got, want)
        print(f'fargan probe {name} {dtype} mode {mode} batch {batch}: ' +
              ', '.join(f'{k} {v:.2e}' for k, v in errors.items()))
        # the previous samples ARE the given ones shifted and this audio
        assert torch.equal(previous[:, 0, 256:], audio)
        assert torch.equal(
            previous[:, 0, :256].cpu(), world.table[batch][2][:, 0, 256:])
        for label, error in errors.items():
            kind = 'audio' if label in ('audio', 'previous') else 'states'
            ledger = 'fargan_probe_init_' if name == 'init' else 'fargan_probe_'
            check(error, probe.GATES[name][kind][dtype],
                  f'{ledger}{kind}:{dtype}', (name, mode, batch, label))


# (batch, frames, seed): the shapes of the reference goldens
FORWARD_SHAPES = {'b2_t8': (2, 8, 41), 'b1_t60': (1, 60, 42),
                  'b3_t25': (3, 25, 43)}
RAGGED = [9, 1, 14, 5, 14, 3] * 6 + [7]           # 37 utterances


@pytest.fixture(scope='module')
def forward_oracle(world):
    """(shape, dtype) -> features, globals and the float64 oracle's audio,
    previous samples and states on the rounded random-init weights."""
    cache = {}

    def get(shape, dtype):
        if (shape, dtype) not in cache:
            batch, frames, seed = FORWARD_SHAPES.get(
                shape, (len(RAGGED), max(RAGGED), 44))
            features, g = fargan_step_oracle.features(
                batch, frames, world.states['init'], seed=seed)
            cache[shape, dtype] = (features, g) + probe.run_oracle_stream(
                world.rounded('init', dtype), features, g)
        return cache[shape, dtype]
    return get


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_forward_against_rounded_oracle(
    device, world, forward_oracle, dtype, mode
):
    """Full `forward` from zero state at random init, as
    test_gpu_fargan.py::test_matches_reference_golden, but against the oracle
    on the stored weights: the f16 and 'mixed' gates no longer hold the
    storage rounding (6.7e-5 and 5.8e-6 on these shapes, of those tests' 2.3e-4
    and 1.8e-5)."""
    model = world.model('init', dtype, mode)
    for shape in FORWARD_SHAPES:
        features, g, want, _, _ = forward_oracle(shape, dtype)
        with torch.inference_mode():
            got = model(features.to(device), g[..., None].to(device), None)
        assert got.shape == want.shape
        error = max_abs(got, want)
        print(f'fargan probe forward {dtype} mode {mode} {shape}: {error:.2e}')
        check(error, probe.FORWARD_GATES[dtype],
              f'fargan_probe_forward:{dtype}', (shape, mode))
    # 37 ragged utterances (two in lockstep per cluster): each its own prefix
    features, g, want, _, _ = forward_oracle('ragged', dtype)
    with torch.inference_mode():
        got = model.forward_channels_last(
            to_cl(features, 128).to(device), g[..., None].to(device), None,
            lengths=RAGGED)
    assert got.shape == want.shape
    error = 0.
    for item, length in enumerate(RAGGED):
        error = max(error, max_abs(got[item, :, :length * 256],
                                   want[item, :, :length * 256]))
        assert not got[item, :, length * 256:].any()
    print(f'fargan probe forward {dtype} mode {mode} ragged: {error:.2e}')
    check(error, probe.FORWARD_GATES[dtype], f'fargan_probe_forward:{dtype}',
          ('ragged', mode))


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_states_against_rounded_oracle(
    device, world, forward_oracle, dtype, mode
):
    """10 frames from zero state: the returned states and previous samples,
    as test_gpu_fargan_stream.py::test_zero_state_equals_forward_and_oracle,
    in all three storage types."""
    model = world.model('init', dtype, mode)
    features, g, _, _, _ = forward_oracle('b3_t25', dtype)
    features = features[:, :, :10]
    _, want_previous, want_states = probe.run_oracle_stream(
        world.rounded('init', dtype), features, g)
    with torch.inference_mode():
        _, previous, states = model.stream(features.to(device), g.to(device))
    errors = {'previous': max_abs(previous, want_previous)}
    for label, got, want in zip(STATES, states, want_states):
        errors[label] = max_abs(got, want)
    print(f'fargan probe stream {dtype} mode {mode}: ' +
          ', '.join(f'{k} {v:.2e}' for k, v in errors.items()))
    for label, error in errors.items():
        kind = 'audio' if label == 'previous' else 'states'
        check(error, probe.STREAM_GATES[kind][dtype],
              f'fargan_probe_stream_{kind}:{dtype}', (mode, label))


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(
        torch.equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_relations_at_trained_scale(device, world, dtype, mode):
    """No gate: in a batch of 37 or 70 (two or four utterances in lockstep
    per cluster, streamed weight slices) row 5 equals the same row run alone
    (one per cluster, LDS-resident slices); two runs are identical; `step`
    equals `stream` on the same frame."""
    model = world.model('trained', dtype, mode)
    alone = world.step(model, 70, rows=slice(5, 6))
    for batch in (37, 70):
        full = world.step(model, batch)
        assert same(full, world.step(model, batch))
        assert same(tuple(t[5:6] if torch.is_tensor(t) else
                          tuple(s[5:6] for s in t) for t in full), alone)
    features, g, previous, states = world.table[37]
    with torch.inference_mode():
        audio, previous, states = model.stream(
            features[:, :, None].to(device), g.to(device), previous.to(device),
            tuple(s.to(device) for s in states))
    assert same((audio[:, 0], previous, states), world.step(model, 37))
