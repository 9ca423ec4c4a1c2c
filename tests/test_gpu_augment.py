"""pm_resample_interp and data augmentation on the device.

Accuracy is held to the bound derived in tests/test_cpu_augment.py,
(K + 5) 2^-24 sum_k |w_k| |x_k| for K = taps, against the float64 evaluation
of the contract with unrounded tables. Every other check is bit for bit: the
fp32 chain of tests/resampy_oracle.py on real tables, exact integer sums on
integer tables, and a sample's independence of the tile, the batch, the memory
layout and a graph replay. The kernel has ONE variant (pm_resample_interp.h
instantiates nothing else), so every case here runs it.
"""
import functools

import numpy as np
import pytest
import torch

import promonet_amd
from promonet_amd import _lib, resampy

import resampy_oracle as oracle
from resample_oracle import first_difference
from test_cpu_augment import BOUND_C, U, slope_holds, write_wav

pytestmark = pytest.mark.gpu

X_PAD, OUT_PAD, TAIL = 7, 5, 3


@functools.lru_cache(maxsize=None)
def product_tables(orig, new):
    return resampy.tables(orig, new)


@functools.lru_cache(maxsize=None)
def reference(orig, new, length, seed=0):
    """(x, the fp32 chain of x) for one row, computed once and shared"""
    x = oracle.signal(length, seed)
    win, delta = product_tables(orig, new)
    want = oracle.chain32(x, orig, new, win, delta)
    want.setflags(write=False)
    x.setflags(write=False)
    return x, want


def run(device, rows, lengths, rates, tables, n_in, n_out):
    """pm_resample_interp through the C entry. rows: arrays of up to n_in
    samples; NaN fills x past every row's end and all of out before the call.
    Returns out (rows, n_out + OUT_PAD) on the host."""
    count = len(rows)
    x = torch.full((count, n_in + X_PAD), float('nan'))
    for row, samples in enumerate(rows):
        x[row, :len(samples)] = torch.from_numpy(
            np.array(samples, dtype=np.float32))
    x = x.to(device)
    out = torch.full((count, n_out + OUT_PAD), float('nan'), device=device)
    meta = torch.tensor(
        [lengths, [rate[0] for rate in rates], [rate[1] for rate in rates]],
        dtype=torch.int32).to(device)
    win, delta = (torch.as_tensor(np.asarray(table, dtype=np.float32)).to(
        device) for table in tables)
    assert oracle.TILE == _lib.lib().pm_resample_interp_tile(*rates[0])
    _lib.check(_lib.lib().pm_resample_interp(
        x.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
        meta[2].data_ptr(), win.data_ptr(), delta.data_ptr(), out.data_ptr(),
        count, n_in, n_in + X_PAD, n_out, n_out + OUT_PAD, _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu()


# ---------------------------------------------------------------------------
# 1. Accuracy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('orig,new', oracle.PAIRS)
def test_accuracy_against_float64(device, orig, new):
    worst = 0.
    for rows in (1, 3):
        for length in oracle.lengths_of(orig, new):
            x = np.stack([oracle.signal(length, seed) for seed in range(rows)])
            got = resampy.resample(torch.from_numpy(x).to(device), orig, new)
            assert got.shape == (rows, length * new // orig)
            got = got.cpu().numpy().astype(np.float64)
            for row in range(rows):
                want, scale, slope, taps, _ = oracle.contract64(
                    x[row], orig, new)
                if length > 2:
                    assert slope_holds(scale, slope)
                bound = (taps + BOUND_C) * U * scale
                error = np.abs(got[row] - want)
                if error.size:
                    worst = max(worst, (error / np.maximum(
                        bound, 1e-300)).max())
                assert (error <= bound).all(), (rows, length, row)
    print(f'{orig} -> {new}: worst error / bound {worst:.3f}')


# ---------------------------------------------------------------------------
# 2. Exact, real tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('orig,new', oracle.PAIRS)
def test_exact_on_real_tables(device, orig, new):
    tables = product_tables(orig, new)
    for length in oracle.lengths_of(orig, new):
        x, want = reference(orig, new, length)
        n_out = want.shape[0] + TAIL
        got = run(device, [x], [length], [(orig, new)], tables, length, n_out)
        expect = np.full((1, n_out + OUT_PAD), np.nan, dtype=np.float32)
        expect[0, :n_out] = 0.
        expect[0, :want.shape[0]] = want
        assert first_difference(got.numpy(), expect, new) is None, length


def test_exact_in_one_mixed_batch(device):
    """Rows of all six pairs, one length each, and an empty row, in one call
    with per-row rates"""
    rows, rates, lengths = [], [], []
    for at, (orig, new) in enumerate(oracle.PAIRS):
        length = oracle.lengths_of(orig, new)[at + 1]
        rows.append(reference(orig, new, length)[0])
        rates.append((orig, new))
        lengths.append(length)
    rows.append(oracle.signal(50))
    rates.append((48000, 22050))
    lengths.append(0)
    n_in = max(lengths)
    x = torch.full((len(rows), n_in), float('nan'))
    for row, samples in enumerate(rows):
        x[row, :len(samples)] = torch.from_numpy(np.array(samples))
    x[-1] = 1.
    got, out_lengths = resampy.resample(
        x.to(device), [rate[0] for rate in rates],
        [rate[1] for rate in rates], lengths=lengths)
    got = got.cpu().numpy()
    assert got.shape[1] == max(n_in * new // orig for orig, new in rates)
    for row, (orig, new) in enumerate(rates[:-1]):
        want = reference(orig, new, lengths[row])[1]
        assert out_lengths[row] == want.shape[0]
        assert np.array_equal(got[row, :want.shape[0]], want), (orig, new)
        assert not got[row, want.shape[0]:].any()
    assert out_lengths[-1] == 0 and not got[-1].any()


# ---------------------------------------------------------------------------
# 3. Exact, integers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('orig,new', oracle.INTEGER_PAIRS)
def test_exact_on_integers(device, orig, new):
    lengths = oracle.lengths_of(orig, new)
    for n_in in (lengths[0], lengths[3], lengths[-2], lengths[-1]):
        x, win, delta = oracle.integer_case(orig, new, 3, n_in)
        row_lengths = [n_in, 0, lengths[lengths.index(n_in) - 1]]
        n_out = n_in * new // orig + TAIL
        got = run(device, list(x), row_lengths, [(orig, new)] * 3,
                  (win, delta), n_in, n_out).numpy().astype(np.float64)
        want = np.full_like(got, np.nan)
        for row, length in enumerate(row_lengths):
            want[row, :n_out] = oracle.integer_outputs(
                x[row], win, delta, orig, new, length, n_out)
        assert first_difference(got, want, new) is None, n_in


def test_refused_rates_answer_nan(device):
    """Rates are device data: a row the kernel cannot take is answered with
    NaN in out[0, n_out), its neighbours are served, nothing else is touched"""
    x, win, delta = oracle.integer_case(48, 64, 4, 40)
    rates = [(48, 64), (8, 1), (0, 5), (64, 48)]
    got = run(device, list(x), [40] * 4, rates, (win, delta), 40, 60).numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    for row in (0, 3):
        orig, new = rates[row]
        want = oracle.integer_outputs(x[row], win, delta, orig, new, 40, 60)
        assert np.array_equal(got[row, :60], want)
        assert np.isnan(got[row, 60:]).all()


# ---------------------------------------------------------------------------
# 4. Independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('orig,new', oracle.PAIRS)
def test_rows_and_delays_are_independent(device, orig, new):
    lengths = oracle.lengths_of(orig, new)
    n_in = lengths[-1]
    x = torch.from_numpy(np.stack(
        [oracle.signal(n_in, seed) for seed in range(4)])).to(device)
    row_lengths = [n_in, lengths[3], lengths[-2], 0]
    batch, out_lengths = resampy.resample(
        x, orig, new, lengths=row_lengths)
    for row, length in enumerate(row_lengths):
        alone = resampy.resample(x[row, :length], orig, new)
        assert out_lengths[row] == alone.shape[0] == length * new // orig
        assert torch.equal(batch[row, :alone.shape[0]], alone), row
        assert not batch[row, alone.shape[0]:].any()
    # a delay by whole periods of the phase, across the first tile's edge
    length = lengths[-2]
    assert length * new // orig >= oracle.TILE
    zeros, delay = oracle.gcd_delay(orig, new, 3)
    assert delay % oracle.TILE != 0
    plain = resampy.resample(x[0, :length], orig, new)
    delayed = resampy.resample(
        torch.cat([x.new_zeros(zeros), x[0, :length]]), orig, new)
    assert torch.equal(delayed[delay:delay + plain.shape[0]], plain)
    # a transposed view and a float64 tensor: the bits of the fp32 copy
    small = x[:3, :lengths[3]].contiguous()
    want = resampy.resample(small, orig, new)
    view = small.T.contiguous().T
    assert not view.is_contiguous()
    assert torch.equal(resampy.resample(view, orig, new), want)
    assert torch.equal(resampy.resample(small.double(), orig, new), want)
    assert torch.equal(
        resampy.resample(small.cpu().reshape(3, 1, -1), orig, new, gpu=0),
        want.reshape(3, 1, -1))


# ---------------------------------------------------------------------------
# 5. Graph
# ---------------------------------------------------------------------------
def test_graph_replay_with_other_rates(device):
    """One captured launch; the replay reads other samples, lengths and
    per-row rates from the same buffers (rates that share the table: every
    upsampling ratio does)"""
    library = _lib.lib()
    first = [(22050, 44100), (24000, 48000), (16000, 22050)]
    second = [(16000, 22050), (11025, 48000), (22050, 44100)]
    n_in, n_out = 700, 700 * 48000 // 11025
    win, delta = resampy.device_tables(1., device)

    def buffers(rates, lengths, seed):
        x = torch.from_numpy(np.stack(
            [oracle.signal(n_in, seed + row) for row in range(3)]))
        meta = torch.tensor(
            [lengths, [rate[0] for rate in rates],
             [rate[1] for rate in rates]], dtype=torch.int32)
        return x.to(device), meta.to(device)

    x, meta = buffers(first, [700, 300, 1], 0)
    out = torch.full((3, n_out), float('nan'), device=device)

    def launch(x, meta, out):
        _lib.check(library.pm_resample_interp(
            x.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
            meta[2].data_ptr(), win.data_ptr(), delta.data_ptr(),
            out.data_ptr(), 3, n_in, n_in, n_out, n_out, _lib.stream()))

    launch(x, meta, out)                                        # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(x, meta, out)
    other_x, other_meta = buffers(second, [2, 700, 699], 10)
    want = torch.full((3, n_out), float('nan'), device=device)
    launch(other_x, other_meta, want)
    x.copy_(other_x)
    meta.copy_(other_meta)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    for row, ((orig, new), length) in enumerate(zip(second, [2, 700, 699])):
        alone = resampy.resample(other_x[row, :length], orig, new)
        assert torch.equal(out[row, :alone.shape[0]], alone)
        assert not out[row, alone.shape[0]:].any()


# ---------------------------------------------------------------------------
# 6. API
# ---------------------------------------------------------------------------
def two_passes(audio, rate, ratio):
    """pitch.from_audio by the oracle's chain"""
    rows = []
    for row in audio.numpy():
        first = int(ratio * rate)
        row = oracle.chain32(row, first, rate, *product_tables(first, rate))
        rows.append(oracle.chain32(
            row, rate, 22050, *product_tables(rate, 22050)))
    return torch.from_numpy(np.stack(rows))


def test_pitch_from_audio_is_two_passes(device):
    audio = torch.from_numpy(
        np.stack([oracle.signal(300, 1), oracle.signal(300, 2)]))
    for ratio in (1.2345, .5, 2.):
        got = promonet_amd.data.augment.pitch.from_audio(
            audio.to(device), 44100, ratio)
        want = two_passes(audio, 44100, ratio)
        assert got.is_cuda and got.shape == want.shape
        assert torch.equal(got.cpu(), want), ratio
    assert int(1.2345 * 44100) == 54441


def test_loudness_from_audio(device):
    loudness = promonet_amd.data.augment.loudness
    audio = torch.from_numpy(oracle.signal(400))[None] * .9
    # peak 0.9 and ratio 2 clip: the ratio is drawn again, as on the host
    torch.manual_seed(5)
    host, host_ratio = loudness.from_audio(audio, 44100, torch.tensor(2.))
    torch.manual_seed(5)
    got, ratio = loudness.from_audio(audio, 44100, torch.tensor(2.), gpu=0)
    assert ratio == host_ratio and ratio != 2. and ratio * .9 < 1.
    assert got.is_cuda and got.shape == host.shape == (1, 200)
    # the audio is the oracle's resample of the device's shift, bit for bit,
    # and the host flow's up to the rounding of the gain 2^(dB / 10)
    shifted = promonet_amd.preprocess.loudness.shift(
        audio.to(device), promonet_amd.convert.ratio_to_db(float(ratio)))
    want = oracle.chain32(
        shifted[0].cpu().numpy(), 44100, 22050, *product_tables(44100, 22050))
    assert np.array_equal(got[0].cpu().numpy(), want)
    # (two gains within 2 ulp of each other; sum_k |w_k| < 4 for this filter)
    assert torch.allclose(got.cpu(), host, rtol=0, atol=16 * U)
    # a ratio that does not clip comes back as it is
    got, ratio = loudness.from_audio(audio, 44100, .75, gpu=0)
    assert ratio == .75
    assert got.abs().max() < .9


def test_pitch_files_are_the_one_file_loop(device, tmp_path):
    pitch = promonet_amd.data.augment.pitch
    files = [tmp_path / f'{i:06d}-100.wav' for i in range(4)]
    for i, (rate, samples, channels) in enumerate(
            [(16000, 310, 1), (44100, 420, 2), (16000, 150, 1),
             (44100, 333, 1)]):
        write_wav(files[i], rate, samples, i, channels)
    ratios = torch.tensor([.5, 2., 1.2345, .8])
    batch = [tmp_path / f'batch{i}.wav' for i in range(4)]
    loop = [tmp_path / f'loop{i}.wav' for i in range(4)]
    pitch.from_files_to_files(files, batch, ratios, gpu=0)
    for file, output, ratio in zip(files, loop, ratios):
        pitch.from_file_to_file(file, output, ratio, gpu=0)
    for i in range(4):
        assert batch[i].read_bytes() == loop[i].read_bytes(), i
    rate, audio = promonet_amd.load.decode(batch[1])
    assert rate == 22050 and audio.shape == (
        2, (420 * 44100 // 88200) * 22050 // 44100)
    # and the oracle's two passes, from the decoded file
    rate, source = promonet_amd.load.decode(files[2])
    rate, audio = promonet_amd.load.decode(batch[2])
    assert torch.equal(audio, two_passes(source, 16000, ratios[2]))
