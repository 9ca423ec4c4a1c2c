"""Ragged batches of the Vocos mel vocoder (pm_vocos_forward_ragged): every
utterance of a zero-padded batch equals its stand-alone synthesis BIT FOR BIT
in every operand type, the padding is never read, `lengths` is read on the
device only, and the batched file entry writes the bytes the one-file loop
writes.

The one tolerance here is the oracle check's: fp32 max-abs against the CPU
restatement (tests/vocos_oracle.py) of the shortest and the longest utterance
of the full-size batch, measured 1.9e-7 on MI355X with PM_RECORD_ERRORS=1
(DESIGN.md sections 2 and 9) and gated at 5.7e-7 (3x), tighter than the
stand-alone FULL_GATE[('fp32', 'init')] = 6.7e-7 of tests/test_gpu_vocos.py.
"""
import pytest
import torch

import promonet_amd
from util import check
import vocos_oracle as oracle

pytestmark = pytest.mark.gpu

# (restated from tests/test_gpu_vocos.py)
BASELINE = dict(MODEL='vocos', SPECTROGRAM_ONLY=True, AUGMENT_PITCH=False,
                AUGMENT_LOUDNESS=False, VOCOS_LAYERS=8)
RESTORE = dict(MODEL='hifigan', SPECTROGRAM_ONLY=False, AUGMENT_PITCH=True,
               AUGMENT_LOUDNESS=True, VOCOS_LAYERS=6)
DTYPES = ('fp32', 'f16', 'bf16')
HOP = 256
ORACLE_GATE = 5.7e-7

# packed offsets 0, 130, 131, 133, 136, 203, 332, 396: utterance ends inside
# the 64-row GEMM tiles and inside both block tiles (128 and 64 rows); the
# 1-3-frame utterances have fewer frames than the overlap-add sums
FRAMES = 130
LENGTHS = [130, 1, 2, 3, 67, 129, 64, 5]


@pytest.fixture
def baseline():
    promonet_amd.configure(**BASELINE)
    yield
    promonet_amd.configure(
        COMPUTE_DTYPE=promonet_amd.config.DEFAULT_COMPUTE_DTYPE, **RESTORE)


def vocos_model(state, device, dtype='fp32'):
    promonet_amd.configure(COMPUTE_DTYPE=dtype)
    model = promonet_amd.model.Vocos(80, 256)
    model.load_state_dict(state)
    return model.to(device)


def padded(mels, lengths, fill=0.):
    mels = mels.clone()
    for b, length in enumerate(lengths):
        mels[b, :, length:] = fill
    return mels


def global_features(g, mode):
    return {'each': g, 'broadcast': g[:1], 'none': None}[mode]


def assert_equals_alone(model, ragged, mels, g, lengths, rows=None):
    """ragged[b] is utterance b synthesised alone, then exact zeros"""
    for b in (range(len(lengths)) if rows is None else rows):
        length = lengths[b]
        own = None if g is None else g[b:b + 1] if g.shape[0] > 1 else g
        alone = model(mels[b:b + 1, :, :length].contiguous(), own)
        assert alone.shape == (1, 1, HOP * length)
        assert torch.equal(ragged[b, :, :HOP * length], alone[0]), \
            (b, length, (ragged[b, :, :HOP * length] - alone[0]).abs().max())
        assert not ragged[b, :, HOP * length:].any(), (b, length)


@pytest.fixture(scope='module')
def small():
    gen = torch.Generator().manual_seed(11)
    mels = torch.randn(len(LENGTHS), 80, FRAMES, generator=gen) - 4.
    g = torch.randn(len(LENGTHS), 256, 1, generator=gen)
    return mels, g, oracle.random_state_vocos(11)


@pytest.mark.parametrize('gmode', ['each', 'broadcast', 'none'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_ragged_batch_is_exact(device, baseline, small, dtype, gmode):
    mels, g, state = small
    model = vocos_model(state, device, dtype)
    mels = padded(mels, LENGTHS).to(device)
    g = global_features(g.to(device), gmode)
    with torch.no_grad():
        ragged = model(mels, g, lengths=LENGTHS)
        assert ragged.shape == (len(LENGTHS), 1, HOP * FRAMES)
        assert_equals_alone(model, ragged, mels, g, LENGTHS)
        # a device tensor of lengths is the same call
        on_device = model(mels, g, lengths=torch.tensor(LENGTHS).to(device))
        assert torch.equal(on_device, ragged)


@pytest.mark.parametrize('dtype', DTYPES)
def test_padding_is_never_read(device, baseline, small, dtype):
    mels, g, state = small
    model = vocos_model(state, device, dtype)
    g = g.to(device)
    with torch.no_grad():
        zeros = model(padded(mels, LENGTHS).to(device), g, lengths=LENGTHS)
        nans = model(padded(mels, LENGTHS, float('nan')).to(device), g,
                     lengths=LENGTHS)
    assert torch.isfinite(nans).all()
    assert torch.equal(zeros, nans)


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_lengths_equal_the_uniform_path(device, baseline, small,
                                                dtype):
    mels, g, state = small
    model = vocos_model(state, device, dtype)
    mels, g = mels.to(device), g.to(device)
    with torch.no_grad():
        uniform = model(mels, g).clone()
        ragged = model(mels, g, lengths=[FRAMES] * len(LENGTHS))
    assert torch.equal(uniform, ragged)


@pytest.fixture(scope='module')
def full_size():
    """batch 32 x 861 frames, lengths from a fixed seed in [215, 861] with one
    forced to 861; the state of test_gpu_vocos.py's full-size test"""
    gen = torch.Generator().manual_seed(21)
    mels = torch.randn(32, 80, 861, generator=gen) - 4.
    g = torch.randn(32, 256, 1, generator=gen)
    lengths = torch.randint(215, 862, (32,), generator=gen).tolist()
    lengths[13] = 861
    assert min(lengths) >= 215 and max(lengths) == 861
    shortest = lengths.index(min(lengths))
    longest = lengths.index(861)
    return (padded(mels, lengths), g, lengths, shortest, longest,
            oracle.random_state_vocos(21))


@pytest.mark.parametrize('dtype', DTYPES)
def test_full_size_is_exact(device, baseline, full_size, dtype):
    mels, g, lengths, shortest, longest, state = full_size
    model = vocos_model(state, device, dtype)
    mels, g = mels.to(device), g.to(device)
    with torch.no_grad():
        ragged = model(mels, g, lengths=lengths)
        assert ragged.shape == (32, 1, HOP * 861)
        assert torch.isfinite(ragged).all()
        assert_equals_alone(model, ragged, mels, g, lengths,
                            rows=sorted({0, 31, shortest, longest}))


def test_full_size_ends_against_the_oracle(device, baseline, full_size):
    mels, g, lengths, shortest, longest, state = full_size
    model = vocos_model(state, device, 'fp32')
    with torch.no_grad():
        ragged = model(mels.to(device), g.to(device), lengths=lengths).cpu()
        for b in (shortest, longest):
            length = lengths[b]
            want = oracle.vocos(mels[b:b + 1, :, :length], g[b:b + 1], state)
            got = ragged[b:b + 1, :, :HOP * length]
            assert got.shape == want.shape
            error = (got - want).abs().max().item()
            print(f'ragged fp32 utterance {b} ({length} frames): max-abs '
                  f'{error:.3e}, peak {want.abs().max().item():.3e}')
            check(error, ORACLE_GATE, 'vocos ragged fp32 abs', b)


def test_lengths_are_read_on_the_device(device, baseline, small):
    """One captured ragged forward replayed with other lengths follows them:
    nothing in the call read `lengths` on the host."""
    mels, g, state = small
    model = vocos_model(state, device, 'bf16')
    first = [5, 9, 1, 12]
    second = [12, 2, 7, 3]
    with torch.inference_mode(False), torch.no_grad():
        # (no zero padding: whatever lies past an end is not read)
        static_mels = mels[:4, :, :12].contiguous().to(device)
        static_g = g[:4].to(device)
        static_lengths = torch.tensor(first, dtype=torch.int32).to(device)
        eager = model(static_mels, static_g, lengths=static_lengths).clone()
        # a workspace of the graph's own, allocated inside the capture
        shared = model._workspace
        with model.private_workspace() as holder:
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                output = model(static_mels, static_g, lengths=static_lengths)
        private = holder.tensor
        assert model._workspace is shared
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(output, eager)
        static_lengths.copy_(torch.tensor(second, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        replayed = output.clone()
        assert private is not None and private is not shared
        assert not torch.equal(replayed, eager)
        assert_equals_alone(model, replayed, static_mels, static_g, second)


@pytest.mark.parametrize('dtype', DTYPES)
def test_mel_generator_with_lengths(device, baseline, dtype):
    promonet_amd.configure(COMPUTE_DTYPE=dtype)
    torch.manual_seed(3)
    model = promonet_amd.model.MelGenerator().to(device)
    gen = torch.Generator().manual_seed(4)
    lengths = [70, 3, 33, 64, 1]
    spectrograms = padded(
        torch.rand(5, 513, 70, generator=gen) + 1e-3, lengths).to(device)
    speakers = torch.tensor([1, 2, 3, 4, 5], device=device)
    balance = torch.tensor([1., .9, 1.1, 1., 1.2], device=device)
    loudness = torch.tensor([1., 1.1, .9, 1.3, 1.], device=device)
    with torch.no_grad():
        ragged = model(spectrograms, speakers, balance, loudness,
                       lengths=lengths)
        assert ragged.shape == (5, 1, HOP * 70)
        for b, length in enumerate(lengths):
            alone = model(
                spectrograms[b:b + 1, :, :length].contiguous(),
                speakers[b:b + 1], balance[b:b + 1], loudness[b:b + 1])
            assert torch.equal(ragged[b, :, :HOP * length], alone[0]), b
            assert not ragged[b, :, HOP * length:].any(), b


def test_batched_files_equal_the_file_loop(device, baseline, tmp_path):
    import numpy as np
    import scipy.io.wavfile
    promonet_amd.configure(COMPUTE_DTYPE='checkpoint')
    gen = torch.Generator().manual_seed(6)
    sources, loop, batched = [], [], []
    for index, (rate, samples) in enumerate([
            (22050, 9000), (44100, 30000), (22050, 2600), (44100, 11111),
            (22050, 20000)]):
        wave = torch.randn(samples, generator=gen) * 0.1
        sources.append(tmp_path / f'in{index}.wav')
        scipy.io.wavfile.write(
            sources[-1], rate, (wave.numpy() * 3e4).astype(np.int16))
        loop.append(tmp_path / f'loop{index}.wav')
        batched.append(tmp_path / f'batched{index}.wav')
    speakers = [3, 0, 7, 1, 2]
    mels = promonet_amd.baseline.mels
    mels.from_files_to_files(sources, loop, speakers, gpu=0)
    mels.from_files_to_files_batched(
        sources, batched, speakers, gpu=0, batch_size=3)
    sizes = set()
    for one, other in zip(loop, batched):
        assert one.read_bytes() == other.read_bytes(), one.name
        rate, data = scipy.io.wavfile.read(other)
        assert rate == promonet_amd.SAMPLE_RATE
        assert data.shape[0] % HOP == 0 and data.shape[0] > 0
        sizes.add(data.shape[0])
    assert len(sizes) == 5
