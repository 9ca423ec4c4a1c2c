"""The device resampler (pm_resample) and its callers.

Accuracy is held to the bound of tests/test_cpu_resample.py, (K + 2) 2^-24
sum_k |h_k| |x_k| for K = taps, against the float64 convolution of the fp32
bank (`load.resample_bank`, itself pinned against the formula there). Every
other check is bit for bit: a sample's bits depend on its own row and index
only, not on the tile, the batch, `lengths`, the memory layout of the input
or a graph replay.
"""
import math

import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd import load
from test_cpu_resample import PAIRS, geometry, lengths_of, signal

pytestmark = pytest.mark.gpu


def convolution64(x, orig_freq, new_freq):
    """(value, sum of absolute products, taps) of rows x (R, n), in float64
    from the fp32 bank"""
    kernels, orig, new, width = load.resample_bank(orig_freq, new_freq)
    bank = kernels[:, 0].to(torch.float64)
    length, taps = x.shape[-1], bank.shape[-1]
    n = torch.arange(-(-new * length // orig))[:, None]
    m = (n // new) * orig - width + torch.arange(taps)[None]
    inside = (m >= 0) & (m < length)
    taken = x.to(torch.float64)[:, m.clamp(0, length - 1)] * inside
    products = taken * bank[(n % new)[:, 0]]
    return products.sum(-1), products.abs().sum(-1), taps


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_bound_on_the_device(device, orig_freq, new_freq):
    orig, new, _, _ = geometry(orig_freq, new_freq)
    worst = 0.
    for length in lengths_of(orig_freq, new_freq):
        x = torch.stack([signal(length, seed) for seed in range(6)])
        want, scale, taps = convolution64(x, orig_freq, new_freq)
        bound = (taps + 2) * 2. ** -24 * scale
        target = -(-new * length // orig)
        for rows in (x[:1], x[:3], x.reshape(2, 3, length)):
            got = load.resample(rows.to(device), orig_freq, new_freq)
            assert got.is_cuda and got.dtype == torch.float32
            assert got.shape == rows.shape[:-1] + (target,)
            got = got.cpu().reshape(-1, target).to(torch.float64)
            error = (got - want[:got.shape[0]]).abs()
            ratio = (error / bound[:got.shape[0]]).max().item()
            worst = max(worst, ratio)
            assert (error <= bound[:got.shape[0]]).all(), (length, ratio)
    print(f'{orig_freq} -> {new_freq}: worst error / bound {worst:.3f}')


@pytest.mark.parametrize('orig_freq,new_freq', [(48000, 22050), (44100, 22050)])
def test_ragged_rows_equal_their_own_calls(device, orig_freq, new_freq):
    orig, new, _, _ = geometry(orig_freq, new_freq)
    strides, _ = load.resample_tile(orig_freq, new_freq)
    n = (strides + 1) * orig + 5            # a tile, a stride and a bit
    lengths = [n, 0, 1, orig, orig + 1, n - 1, 5 * orig - 1]
    x = torch.stack([signal(n, seed) for seed in range(len(lengths))])
    x = x.to(device)
    out, out_lengths = load.resample(x, orig_freq, new_freq, lengths=lengths)
    assert out.shape == (len(lengths), -(-new * n // orig))
    assert out_lengths == [-(-new * length // orig) for length in lengths]
    for row, length in enumerate(lengths):
        alone = load.resample(
            x[row:row + 1, :length].contiguous(), orig_freq, new_freq)
        assert alone.shape == (1, out_lengths[row])
        assert torch.equal(out[row, :out_lengths[row]], alone[0]), row
        assert not out[row, out_lengths[row]:].any(), row
    # the padding is never read
    poisoned = x.clone()
    for row, length in enumerate(lengths):
        poisoned[row, length:] = float('nan')
    again, _ = load.resample(poisoned, orig_freq, new_freq, lengths=lengths)
    assert torch.equal(again, out)
    # lengths on the device, and out of range: clamped there to [0, n]
    tensor = torch.tensor(lengths, device=device)
    tensor[1], tensor[0] = -3, n + 100
    clamped, clamped_lengths = load.resample(
        x, orig_freq, new_freq, lengths=tensor)
    assert torch.equal(clamped, out)
    assert clamped_lengths.device == tensor.device
    assert clamped_lengths.tolist() == out_lengths


def test_a_shift_by_whole_strides_is_exact(device):
    orig_freq, new_freq = 48000, 22050
    orig, new, _, _ = geometry(orig_freq, new_freq)
    strides, _ = load.resample_tile(orig_freq, new_freq)
    edge = strides * orig                   # input samples per tile
    # the signal ends half a stride before a tile edge: every shift moves its
    # end, and with it the filter's support, over that edge
    for length in (edge - orig // 2, 3 * edge - orig // 2):
        x = signal(length, 7)[None].to(device)
        base = load.resample(x, orig_freq, new_freq)
        for shift in (1, 3, 17):
            assert (length - 1) // edge != (length - 1 + shift * orig) // edge
            moved = load.resample(
                torch.nn.functional.pad(x, (shift * orig, 0)),
                orig_freq, new_freq)
            assert moved.shape[-1] == base.shape[-1] + shift * new
            # (the samples before are the filter's pre-ringing, not zeros)
            assert torch.equal(moved[:, shift * new:], base), (length, shift)


def test_layouts_and_types(device):
    orig_freq, new_freq = 48000, 22050
    interleaved = torch.stack(
        [signal(2001, 1), signal(2001, 2)], dim=1).to(device)   # (samples, 2)
    view = interleaved.T
    assert not view.is_contiguous()
    want = load.resample(view.contiguous(), orig_freq, new_freq)
    assert torch.equal(load.resample(view, orig_freq, new_freq), want)
    assert torch.equal(
        load.resample(view.to(torch.float64), orig_freq, new_freq), want)
    # rows of a wider matrix: a row stride above the row's length
    wide = torch.zeros(2, 3000, device=device)
    wide[:, :2001] = view
    assert torch.equal(
        load.resample(wide[:, :2001], orig_freq, new_freq), want)
    # empty input: empty output, nothing launched
    assert load.resample(
        torch.zeros(2, 0, device=device), orig_freq, new_freq).shape == (2, 0)
    assert load.resample(
        torch.zeros(0, 9, device=device), orig_freq, new_freq).shape == (0, 5)
    # equal rates: the input itself
    assert load.resample(view, 22050, 22050) is view
    with pytest.raises(ValueError, match='22051 Hz -> 22050 Hz'):
        load.resample(view, 22051, 22050)


def test_graph_replay_with_other_lengths(device):
    orig_freq, new_freq = 48000, 22050
    orig, new, _, _ = geometry(orig_freq, new_freq)
    strides, _ = load.resample_tile(orig_freq, new_freq)
    n = (strides + 1) * orig + 5
    x = torch.stack([signal(n, seed) for seed in range(3)]).to(device)
    lengths = torch.tensor([n, orig + 1, 5 * orig - 1], dtype=torch.int32,
                           device=device)
    load.resample(x, orig_freq, new_freq, lengths=lengths)      # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, out_lengths = load.resample(
            x, orig_freq, new_freq, lengths=lengths)
    other = torch.stack([signal(n, seed) for seed in range(3, 6)]).to(device)
    other_lengths = torch.tensor([7, n, n - orig], dtype=torch.int32,
                                 device=device)
    want, want_lengths = load.resample(
        other, orig_freq, new_freq, lengths=other_lengths)
    x.copy_(other)
    lengths.copy_(other_lengths)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(out_lengths, want_lengths)
    assert want_lengths.tolist() == [
        -(-new * length // orig) for length in (7, n, n - orig)]


def test_preprocess_resamples_on_the_device(device):
    x = signal(48000, 3)[None] * .5
    got = promonet_amd.preprocess.from_audio(
        x, sample_rate=48000, gpu=0, features=['loudness'])
    want = promonet_amd.preprocess.loudness.from_audio(
        load.resample(x.to(device), 48000, promonet_amd.SAMPLE_RATE),
        promonet_amd.LOUDNESS_BANDS)
    assert got.shape == (promonet_amd.LOUDNESS_BANDS, 22050 // 256)
    assert torch.equal(got, want)


BASELINE = dict(MODEL='vocos', SPECTROGRAM_ONLY=True, AUGMENT_PITCH=False,
                AUGMENT_LOUDNESS=False, VOCOS_LAYERS=8)
RESTORE = dict(MODEL='hifigan', SPECTROGRAM_ONLY=False, AUGMENT_PITCH=True,
               AUGMENT_LOUDNESS=True, VOCOS_LAYERS=6)


@pytest.fixture
def baseline():
    """(restated from tests/test_gpu_vocos_ragged.py)"""
    promonet_amd.configure(**BASELINE)
    yield
    promonet_amd.configure(
        COMPUTE_DTYPE=promonet_amd.config.DEFAULT_COMPUTE_DTYPE, **RESTORE)


def test_mels_resamples_on_the_device(device, baseline, monkeypatch):
    mels = promonet_amd.baseline.mels
    x = signal(9000, 4)[None] * .5
    want = mels.from_audio(
        load.resample(x.to(device), 44100, promonet_amd.SAMPLE_RATE), gpu=0)

    def host_resampler(*args, **kwargs):
        raise AssertionError('the host resampler is on the path')
    monkeypatch.setattr(torch.nn.functional, 'conv1d', host_resampler)
    got = mels.from_audio(x, sample_rate=44100, gpu=0)
    assert torch.equal(mels.resample(x.to(device), 44100),
                       load.resample(x.to(device), 44100, 22050))
    monkeypatch.undo()
    assert got.shape == (1, 4500 // 256 * 256)
    assert torch.equal(got, want)


def write_files(folder):
    """A 48 kHz int16 stereo, a 44.1 kHz float32 mono, a 16 kHz int16 mono
    and a 22.05 kHz int16 mono file of 0.1 - 0.4 s"""
    import scipy.io.wavfile
    files = []
    for index, (rate, samples, channels, kind) in enumerate([
            (48000, 9001, 2, np.int16), (44100, 15000, 1, np.float32),
            (16000, 3000, 1, np.int16), (22050, 5000, 1, np.int16)]):
        wave = torch.stack(
            [signal(samples, 10 * index + c) for c in range(channels)], 1)
        wave = (wave * .3).numpy()
        if kind is np.int16:
            wave = (wave * 32767).astype(np.int16)
        files.append(folder / f'in{index}.wav')
        scipy.io.wavfile.write(
            files[-1], rate, wave[:, 0] if channels == 1 else wave)
    return files


def test_files_load_on_the_device(device, tmp_path):
    for file in write_files(tmp_path):
        rate, data = load.decode(file)
        got = load.audio(file, gpu=0)
        want = load.audio(file)
        assert got.is_cuda and got.shape == want.shape
        if rate == promonet_amd.SAMPLE_RATE:
            assert torch.equal(got.cpu(), want)
            continue
        # per channel before the mean: the mean of errors within the bound
        # is within the mean of the bounds
        value, scale, taps = convolution64(
            data.contiguous(), rate, promonet_amd.SAMPLE_RATE)
        bound = ((taps + 2) * 2. ** -24 * scale).mean(0)
        error = (got.cpu()[0].to(torch.float64) - value.mean(0)).abs()
        assert (error <= bound).all(), (file.name, (error / bound).max())
        host = (want[0].to(torch.float64) - value.mean(0)).abs()
        assert (host <= bound).all(), file.name


def test_batched_files_take_one_launch_per_rate(device, baseline, tmp_path):
    promonet_amd.configure(COMPUTE_DTYPE='checkpoint')
    mels = promonet_amd.baseline.mels
    files = write_files(tmp_path)
    # a second 48 kHz file, mono and shorter: one ragged launch with the first
    import scipy.io.wavfile
    files.append(tmp_path / 'in4.wav')
    scipy.io.wavfile.write(
        files[-1], 48000, (signal(7000, 50).numpy() * 9000).astype(np.int16))
    decoded = [load.decode(file) for file in files]
    for file, audio in zip(files, mels._load_batch(decoded, device)):
        assert torch.equal(audio, load.audio(file, gpu=0)), file.name
    loop = [tmp_path / f'loop{index}.wav' for index in range(len(files))]
    batched = [tmp_path / f'batched{index}.wav' for index in range(len(files))]
    speakers = [3, 0, 7, 1, 2]
    mels.from_files_to_files(files, loop, speakers, gpu=0)
    mels.from_files_to_files_batched(
        files, batched, speakers, gpu=0, batch_size=3)
    for one, other in zip(loop, batched):
        assert one.read_bytes() == other.read_bytes(), one.name
        assert len(one.read_bytes()) > 44 + 2 * 256
