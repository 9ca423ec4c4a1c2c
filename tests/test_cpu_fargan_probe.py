"""The FARGAN probe's own footing, checked on the CPU oracle alone: the
teacher-forced cases put the network where a trained one lives and stay
stable there, `rounded_state` rounds what the engine rounds, and every
planted defect moves the float64 oracle far above its arithmetic noise - so
that test_gpu_fargan_probe.py, whose gates sit between the two, would see
it."""
import pytest
import torch

import fargan_probe as probe
import restatement as oracle

DTYPES = ('fp32', 'mixed', 'f16')


@pytest.fixture(scope='module')
def base():
    return probe.base_state()


@pytest.fixture(scope='module')
def table(base):
    return probe.cases(state=base)


@pytest.fixture(scope='module')
def states(base):
    return {name: make(base) for name, make in probe.WEIGHT_SETS.items()}


@pytest.fixture(scope='module')
def noise(states, table):
    """(set, dtype) -> the oracle's fp32-versus-fp64 (audio, states)
    difference on the 70-row table, weights rounded as stored."""
    out = {}
    for name, state in states.items():
        for dtype in DTYPES:
            rounded = probe.rounded_state(state, dtype)
            out[name, dtype] = probe.difference(
                probe.run_oracle(rounded, table[70], torch.float32),
                probe.run_oracle(rounded, table[70]))
    return out


def test_case_table(table):
    """Every period edge, both branches of the lookback wrap, the ranges of
    the given state; the smaller batches are the table's first rows."""
    features, g, previous, given = table[70]
    assert features.shape == (70, 114) and g.shape == (70, 258)
    assert previous.shape == (70, 1, 512)
    assert [tuple(s.shape) for s in given] == [
        (70, n) for n in probe.STATE_SIZES]
    for batch in probe.BATCHES:
        assert table[batch][0].shape[0] == batch
        for small, full in zip(table[batch][:3], table[70][:3]):
            assert torch.equal(small, full[:batch])
        periods = table[batch][0][:, -1]
        assert periods.min() >= 33 and periods.max() <= 510
        rounded = torch.round(periods)
        assert (rounded <= 65).any() and (rounded > 65).any()   # wrap, none
        assert 33. in periods and 510. in periods
    for edge in probe.PERIOD_EDGES:
        assert edge in table[37][0][:, -1] and edge in table[70][0][:, -1]
    # ties go to even, in rintf as in torch.round
    assert torch.round(torch.tensor([64.5, 65.5, 127.5])).tolist() == [
        64., 66., 128.]
    assert previous.abs().max() <= .95 and previous.abs().max() > .9
    assert all(s.abs().max() > .99 and s.abs().max() <= 1 for s in given)


@pytest.mark.parametrize('name', ['trained', 'overflow'])
def test_conditioning(states, table, name):
    """One frame at trained scale is where a trained network lives: GRU
    states up to 1, 5 % of the GRU gate pre-activations beyond +-4, audio
    peak above .5. The overflow set also passes both ends of both
    activations' exponentials (fg_tanh beyond +-45, fg_sigmoid beyond
    +-89)."""
    with probe.preactivations() as taps:
        audio, _, new = probe.run_oracle(states[name], table[70])
    assert len(taps['tanh']) == 3 + 4 * 6 and len(taps['sigmoid']) == 4 * 11
    gates = probe.gru_gate_preactivations(taps)
    assert gates.numel() == 70 * 4 * 3 * 2 * 256
    hidden = max(h.abs().max().item() for h in new[:3])
    beyond = (gates.abs() > 4).double().mean().item()
    peak = audio.abs().max().item()
    tanh = torch.cat([t.flatten() for t in taps['tanh']])
    sigmoid = torch.cat([t.flatten() for t in taps['sigmoid']])
    print(f'{name}: max |h| {hidden:.4f}, gate pre-activations beyond +-4 '
          f'{beyond:.3f}, audio peak {peak:.3f}, tanh in [{tanh.min():.1f}, '
          f'{tanh.max():.1f}], sigmoid in [{sigmoid.min():.1f}, '
          f'{sigmoid.max():.1f}]')
    assert hidden > .9 and beyond >= .05 and peak > .5
    if name == 'overflow':
        assert tanh.min() < -45 and tanh.max() > 45
        assert sigmoid.min() < -89 and sigmoid.max() > 89
        assert all(torch.isfinite(t).all() for t in (audio, *new))


def test_noise_cap(noise):
    """The reference alone holds the cap at every weight set and storage
    type: a frame on which fp32 and fp64 arithmetic part ways further could
    not tell a wrong kernel from a right one."""
    for (name, dtype), (audio, new) in noise.items():
        print(f'oracle fp32 vs fp64, {name} {dtype}: audio {audio:.2e}, '
              f'states {new:.2e}')
    for (name, dtype), (audio, new) in noise.items():
        assert audio <= probe.NOISE_CAP['audio'], (name, dtype, audio)
        assert new <= probe.NOISE_CAP['states'], (name, dtype, new)


def test_rounding_table(states):
    """'f16' rounds all 17 layers, 'mixed' exactly the 11 that
    fargan_layers() marks insensitive; rounded weights are f16 values, the
    others keep the folded fp32 bits; nothing else in the state moves."""
    assert len(probe.LAYERS) == 17 and len(probe.INSENSITIVE) == 11
    assert set(probe.INSENSITIVE) | set(probe.SENSITIVE) == set(probe.LAYERS)
    state = states['trained']
    folded = probe.rounded_state(state, 'fp32')
    weights = oracle.fargan_weights(state)
    for prefix in probe.LAYERS:
        assert prefix + '.weight_g' not in folded
    assert all(torch.equal(a, b) for a, b in zip(
        oracle.fargan_weights(folded).values(), weights.values()))
    for dtype, layers in (('f16', probe.LAYERS), ('mixed', probe.INSENSITIVE)):
        rounded = probe.rounded_state(state, dtype)
        assert rounded.keys() == folded.keys()
        changed = {prefix for prefix in probe.LAYERS if not torch.equal(
            rounded[probe.key(prefix)], folded[probe.key(prefix)])}
        assert changed == set(layers), dtype
        for prefix in probe.LAYERS:
            w = rounded[probe.key(prefix)]
            assert w.dtype == torch.float32
            assert w.shape == folded[probe.key(prefix)].shape
            if prefix in layers:
                assert torch.equal(w.half().float(), w)
                assert (w - folded[probe.key(prefix)]).abs().max() <= \
                    folded[probe.key(prefix)].abs().max() * 2 ** -11
        plain = {probe.key(prefix) for prefix in probe.LAYERS}
        for name in rounded.keys() - plain:     # embeddings, buffers
            assert rounded[name] is state[name]
    # the fold handed in is the fold used
    marked = probe.rounded_state(state, 'mixed', fold=lambda g, v: v * 0 + 3)
    assert (marked[probe.key(probe.FWCONV)] == 3).all()
    # truncation never moves away from zero and differs from rounding
    w = folded[probe.key(probe.GRU[0])]
    cut = probe._truncate(w)
    assert (cut.abs() <= w.abs()).all() and torch.equal(cut.half().float(), cut)
    assert ((w - cut).abs() < w.abs() * 2 ** -10 + 2 ** -24).all()
    assert not torch.equal(cut, w.half().float())


def test_scaled_state(base):
    scaled = probe.scaled_state(base, gru=4., glu=3., dense=2.)
    before, after = oracle.fargan_weights(base), oracle.fargan_weights(scaled)
    factors = {'cond0': 2, 'cond1': 2, 'cond2': 2, 'fwconv': 2, 'skip': 2,
               'out': 2, 'fwconv_glu': 3, 'skip_glu': 3}
    for n in (1, 2, 3):
        factors.update({f'gru{n}_ih': 4, f'gru{n}_hh': 4, f'gru{n}_glu': 3})
    assert factors.keys() == before.keys()
    for name, factor in factors.items():
        assert torch.allclose(after[name], before[name] * factor, rtol=1e-6)
    assert torch.equal(scaled[probe.FWCONV + '.weight_v'],
                       base[probe.FWCONV + '.weight_v'])


def test_sensitivity(states, table, noise):
    """Every planted defect moves the float64 oracle, on the teacher-forced
    frame at trained scale, by at least 20 times its fp32-versus-fp64 noise
    in the output it is meant to show in - and every gate of the GPU test
    lies between the two."""
    state, case = states['trained'], table[70]
    want = {dtype: probe.run_oracle(probe.rounded_state(state, dtype), case)
            for dtype in DTYPES}
    smallest = {}
    print(f'{"defect":24s} {"storage":7s} {"audio":>9s} {"states":>9s} '
          f'{"noise: audio":>13s} {"states":>9s}  shows in')
    rows = []
    for name, (defect, dtypes, shows) in probe.DEFECTS.items():
        for dtype in dtypes:
            got = probe.run_oracle(
                defect(state, dtype, oracle.fold_weight_norm_linear), case)
            effect = dict(zip(('audio', 'states'),
                              probe.difference(got, want[dtype])))
            floor = dict(zip(('audio', 'states'), noise['trained', dtype]))
            print(f'{name:24s} {dtype:7s} {effect["audio"]:9.2e} '
                  f'{effect["states"]:9.2e} {floor["audio"]:13.2e} '
                  f'{floor["states"]:9.2e}  {shows}')
            rows.append((name, dtype, effect[shows], floor[shows]))
            smallest[shows, dtype] = min(
                smallest.get((shows, dtype), 1.), effect[shows])
    for name, dtype, effect, floor in rows:
        assert effect >= 20 * floor, (name, dtype, effect, floor)
    for kind in ('audio', 'states'):
        gates = probe.GATES['trained'][kind]
        assert probe.GATES['overflow'][kind] is gates
        for dtype in DTYPES:
            if (kind, dtype) in smallest:
                assert gates[dtype] < smallest[kind, dtype], (kind, dtype)
            # the init set's errors are smaller; so are its gates
            assert probe.GATES['init'][kind][dtype] <= gates[dtype]
    every = [probe.FORWARD_GATES, *probe.STREAM_GATES.values(),
             *probe.GATES['trained'].values(), *probe.GATES['init'].values()]
    for gates in every:
        assert all(gates[d] <= 4 * gates['fp32'] for d in DTYPES)
