"""The device limiter (pm_limit), the loudness shift (pm_loudness_shift) and
`scale`, their composition.

`limit` is held bit for bit (`torch.equal`, output and gain) to the literal
loop of tests/loudness_edit_oracle.py, which tests/test_cpu_loudness_edit.py
pins against the reference's golden. `shift` is held to the float64 closed
form in units of 2^-24 relative error:

    measured on an MI355X (largest over the shapes below)   3.19, at (40, 10 257)
    torch's own fp32 interpolate on the CPU, (9, 2 321)     9.33

The gate is 3 x the first figure and must not exceed 4 x the second, which
this file recomputes.
"""
import types

import pytest
import torch

import promonet_amd
from promonet_amd.preprocess import loudness
import loudness_edit_oracle as oracle
from test_cpu_loudness_edit import SHIFT_SHAPES, host_shift_units

pytestmark = pytest.mark.gpu

CHUNK, TILE = loudness.limit_tile()
DELAY = 40
LENGTHS = (1, DELAY - 1, DELAY, CHUNK - 1, CHUNK + 1, TILE - 1, TILE + 1,
           2 * TILE + 5)
# units of 2^-24, the largest relative error measured on an MI355X
SHIFT_MEASURED = 3.19
SHIFT_GATE = 3 * SHIFT_MEASURED


@pytest.fixture(scope='module')
def classes():
    return oracle.inputs(CHUNK, TILE)


def check(device, name, length, classes, **parameters):
    x = classes[name] if length is None else classes[name][:, :length]
    want, want_gain = oracle.literal(name, length, CHUNK, TILE, **parameters)
    on_device = x.to(device)
    got, gain, counts = loudness.limit_with_trace(on_device, **parameters)
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got.cpu(), want), (name, length)
    assert torch.equal(gain.cpu()[0], want_gain), (name, length)
    assert torch.equal(loudness.limit(on_device, **parameters), got)
    assert torch.equal(on_device.cpu(), x)          # the input is untouched
    return counts[0].tolist()


@pytest.mark.parametrize('name', oracle.CLASSES)
def test_limit_is_the_literal_loop(device, classes, name):
    for length in LENGTHS + (None,):
        counts = check(device, name, length, classes)
        if name == 'quiet':
            # nothing above the threshold: no serial step, every tile skipped
            steps = (length or classes[name].shape[1]) + DELAY - 1
            assert counts == [0, 0, 0, -(-steps // TILE)]
    if name == 'saturated':
        assert counts[1] >= classes[name].shape[1]


@pytest.mark.parametrize('parameters', [
    dict(delay=1), dict(delay=7), dict(attack_coef=.5),
    dict(release_coef=.99), dict(threshold=.5),
    dict(delay=TILE + 300, attack_coef=.7)])
def test_limit_with_other_parameters(device, classes, parameters):
    # (the last: a delay beyond one tile reads x back from memory)
    length = None if len(parameters) == 1 else TILE + 700
    check(device, 'bursts', length, classes, **parameters)


def ragged(classes):
    n = 2 * TILE + 5
    lengths = [n, 0, 1, DELAY, CHUNK + 1, n - 1, TILE + 1]
    names = ('bursts', 'quiet', 'saturated', 'spike', 'edges', 'settle',
             'bursts')
    x = torch.cat([classes[name][:, :n] for name in names])
    x[6] = x[6].flip(0)
    return x, lengths


def test_ragged_rows_equal_their_own_calls(device, classes):
    x, lengths = ragged(classes)
    n = x.shape[1]
    x = x.to(device)
    out, gain, _ = loudness.limit_with_trace(x, lengths=lengths)
    assert out.shape == x.shape and gain.shape == (7, n + DELAY - 1)
    for row, length in enumerate(lengths):
        one, one_gain, _ = loudness.limit_with_trace(
            x[row:row + 1, :length].contiguous())
        assert torch.equal(out[row, :length], one[0]), row
        assert not out[row, length:].any(), row
        assert torch.equal(gain[row, :length + DELAY - 1], one_gain[0]), row
        assert not gain[row, length + DELAY - 1:].any(), row
    # the padding is never read
    poisoned = x.clone()
    for row, length in enumerate(lengths):
        poisoned[row, length:] = float('nan')
    assert torch.equal(loudness.limit(poisoned, lengths=lengths), out)
    # lengths on the device, and out of range: clamped there to [0, n]
    tensor = torch.tensor(lengths, device=device)
    tensor[1], tensor[0] = -3, n + 100
    assert torch.equal(loudness.limit(x, lengths=tensor), out)
    # another batch order
    order = [3, 6, 0, 5, 1, 4, 2]
    moved = loudness.limit(x[order], lengths=[lengths[i] for i in order])
    assert torch.equal(moved, out[order])
    # full rows: (B, T) against B calls of (1, T), and a second run
    full = loudness.limit(x)
    for row in range(len(lengths)):
        assert torch.equal(full[row:row + 1], loudness.limit(x[row:row + 1]))
    assert torch.equal(loudness.limit(x), full)
    assert torch.equal(full[0], out[0])


def test_layouts_and_types(device, classes):
    x, _ = ragged(classes)
    x = x.to(device)
    want = loudness.limit(x)
    interleaved = x.T.contiguous()                  # (samples, rows)
    assert not interleaved.T.is_contiguous()
    assert torch.equal(loudness.limit(interleaved.T), want)
    assert torch.equal(loudness.limit(x.to(torch.float64)), want)
    # rows of a wider matrix: a row stride above the row's length
    wide = torch.zeros(x.shape[0], x.shape[1] + 100, device=device)
    wide[:, :x.shape[1]] = x
    assert torch.equal(loudness.limit(wide[:, :x.shape[1]]), want)
    assert loudness.limit(torch.zeros(2, 0, device=device)).shape == (2, 0)
    with pytest.raises(promonet_amd._lib.LibraryError, match='delay'):
        loudness.limit(x, delay=0)
    with pytest.raises(promonet_amd._lib.LibraryError, match=r'\(0, 1\)'):
        loudness.limit(x, attack_coef=1.)


def test_graph_replay_with_other_lengths(device, classes):
    x, lengths = ragged(classes)
    n = x.shape[1]
    x = x.to(device)
    lengths = torch.tensor(lengths, dtype=torch.int32, device=device)
    loudness.limit(x, lengths=lengths)              # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = loudness.limit(x, lengths=lengths)
    other = x.flip(0).contiguous()
    other_lengths = torch.tensor(
        [7, n, TILE, 0, n - CHUNK, DELAY - 1, 2 * TILE], dtype=torch.int32,
        device=device)
    want = loudness.limit(other, lengths=other_lengths)
    x.copy_(other)
    lengths.copy_(other_lengths)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_shift_against_the_closed_form(device):
    cap = 4 * host_shift_units()
    assert SHIFT_GATE <= cap, (SHIFT_GATE, cap)
    worst = {}
    for frames, samples in SHIFT_SHAPES:
        audio, value = oracle.shift_inputs(frames, samples)
        got = loudness.shift(audio.to(device), value.to(device))
        assert got.dtype == torch.float32 and got.shape == audio.shape
        worst[frames, samples] = oracle.relative_units(
            got.cpu(), oracle.shift64(audio, value))
    # the scalar path, a Python number and a batch
    audio, _ = oracle.shift_inputs(3, 777, rows=3)
    for value in (-6.5, 0., 11):
        got = loudness.shift(audio.to(device), value)
        worst['scalar', value] = oracle.relative_units(
            got.cpu(), oracle.shift64(audio, value))
    assert torch.equal(loudness.shift(audio.to(device), 0.), audio.to(device))
    # a batch with a contour per row, and one contour for every row
    audio, value = oracle.shift_inputs(9, 2321, rows=3)
    got = loudness.shift(audio.to(device), value.to(device))
    worst['batch'] = oracle.relative_units(
        got.cpu(), oracle.shift64(audio, value))
    got = loudness.shift(audio.to(device), value[:1].to(device))
    worst['shared'] = oracle.relative_units(
        got.cpu(), oracle.shift64(audio, value[:1]))
    for key, units in worst.items():
        print(f'shift {key}: {units:.2f} units of 2^-24')
    print(f'gate {SHIFT_GATE:.2f}, cap {cap:.2f}')
    assert max(worst.values()) <= SHIFT_GATE, worst


def test_shift_ragged_rows_and_graph_replay(device):
    samples, frames = 2321, 9
    audio, value = oracle.shift_inputs(frames, samples, rows=5)
    audio, value = audio.to(device), value.to(device)
    lengths = [samples, 0, 1, 513, samples - 1]
    frame_lengths = [frames, 1, 1, 2, frames - 1]
    out = loudness.shift(audio, value, lengths, frame_lengths)
    units = 0.
    for row, (n, f) in enumerate(zip(lengths, frame_lengths)):
        alone = loudness.shift(audio[row:row + 1, :n].contiguous(),
                               value[row:row + 1, :f].contiguous())
        assert torch.equal(out[row, :n], alone[0]), row
        assert not out[row, n:].any(), row
        if n:
            units = max(units, oracle.relative_units(
                alone.cpu(), oracle.shift64(
                    audio[row:row + 1, :n].cpu(), value[row:row + 1, :f].cpu())))
    assert units <= SHIFT_GATE, units
    # a non-contiguous input and float64
    assert torch.equal(
        loudness.shift(audio.T.contiguous().T.double(), value.double()),
        loudness.shift(audio, value))
    lengths = torch.tensor(lengths, dtype=torch.int32, device=device)
    frame_lengths = torch.tensor(
        frame_lengths, dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = loudness.shift(audio, value, lengths, frame_lengths)
    other_lengths = torch.tensor(
        [5, samples, 700, 0, 2000], dtype=torch.int32, device=device)
    other_frames = torch.tensor(
        [2, frames, 3, 1, 7], dtype=torch.int32, device=device)
    want = loudness.shift(audio.flip(0), value.flip(0), other_lengths,
                          other_frames)
    audio.copy_(audio.flip(0))
    value.copy_(value.flip(0))
    lengths.copy_(other_lengths)
    frame_lengths.copy_(other_frames)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, want)


def scale_audio(rows, peak):
    gen = torch.Generator().manual_seed(163 + rows)
    audio = (torch.rand(rows, 2560, generator=gen) * 2 - 1) * peak
    return torch.where(audio == 0, torch.full_like(audio, .1), audio)


@pytest.mark.parametrize('rows', [1, 3])
def test_scale_is_the_composition(device, rows):
    audio = scale_audio(rows, .9).to(device)
    current = loudness.from_audio(audio)    # (1, 10) or (rows, 1, 10)
    # 8 bands around 30 dB above the audio's own loudness: a ratio near 8,
    # which `shift` takes for 8 dB, a gain near 1.7
    gen = torch.Generator().manual_seed(164)
    bands = torch.rand(8, 10, generator=gen) * 4
    target = current + 28 + bands.to(device)
    assert target.shape == ((8, 10) if rows == 1 else (rows, 8, 10))
    got = loudness.scale(audio, target)
    assert got.shape == audio.shape and got.dtype == torch.float32
    mean = target.mean(dim=-2, keepdim=True)
    ratio = promonet_amd.convert.db_to_ratio(mean - current)
    shifted = loudness.shift(audio, ratio.reshape(rows, -1))
    assert torch.equal(got, loudness.limit(shifted))
    assert (shifted.abs() > .99).any()      # the limiter has work to do
    # the oracle's composition, fed the device's loudness: the shift within
    # its gate, the limiter exact given the device's shift
    want = oracle.shift64(audio.cpu(), ratio.reshape(rows, -1).cpu())
    assert oracle.relative_units(shifted.cpu(), want) <= SHIFT_GATE
    assert torch.equal(got.cpu(), oracle.limit_rows(shifted.cpu())[0])
    assert torch.equal(
        got[:1].cpu(), oracle.limit_literal(shifted[:1].cpu())[0])


def test_scale_to_its_own_loudness_returns_the_audio(device):
    audio = scale_audio(3, .49).to(device)
    current = loudness.from_audio(audio)
    got = loudness.scale(audio, current, reference_gain=False)
    assert oracle.relative_units(got.cpu(), audio.cpu().double()) <= SHIFT_GATE
    # with the reference's double conversion a difference of 0 dB becomes the
    # ratio 1, and that a shift by 1 dB
    quirk = loudness.scale(audio[:1], current[0])
    want = audio[:1].cpu().double() * 2 ** .1
    assert oracle.relative_units(quirk.cpu(), want) <= SHIFT_GATE


def test_the_patch_installs_all_three(device, classes):
    stand_in = types.SimpleNamespace(
        model=types.SimpleNamespace(HiFiGAN=None, FARGAN=None, Generator=None),
        synthesize=types.SimpleNamespace(),
        preprocess=types.SimpleNamespace(
            spectrogram=types.SimpleNamespace(),
            loudness=types.SimpleNamespace(
                from_audio=None, limit=None, scale=None, shift=None)))
    promonet = promonet_amd.patch(stand_in)
    for name in ('from_audio', 'limit', 'scale', 'shift'):
        assert getattr(promonet.preprocess.loudness, name) is \
            getattr(loudness, name)
    x = classes['bursts'].to(device)
    assert torch.equal(promonet.preprocess.loudness.limit(x),
                       loudness.limit(x))
