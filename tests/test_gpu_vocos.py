"""Vocos mel vocoder on the GPU (pm_vocos.hip) against the CPU restatement
(tests/vocos_oracle.py) and the real-reference golden (tests/golden/vocos.pt).

Gates are <= 3x the errors measured with PM_RECORD_ERRORS=1 (DESIGN.md
section 2); the fp32 end-to-end contract (1e-4) is far looser than its gates.

test_istft_against_irfft_and_fold and test_head_exp_clip_and_large_phases
take one maximum over dense outputs, relative to the peak, against an fp32
oracle: they hold the head as a whole, at sizes up to 861 frames. What they
average away is in the care of tests/test_gpu_vocos_head.py: every bin of the
inverse transform on its own samples against a float64 oracle, the expf, the
side of the clip and the phase of bins below the clip, the handoff of the
logits in each operand type with no tolerance, and the index arithmetic of the
overlap-add (frame range, the clamp at the last frame, the crop, the envelope
of the frames that exist) bit for bit.
"""
import math

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from util import check
import vocos_oracle as oracle

pytestmark = pytest.mark.gpu

BASELINE = dict(MODEL='vocos', SPECTROGRAM_ONLY=True, AUGMENT_PITCH=False,
                AUGMENT_LOUDNESS=False, VOCOS_LAYERS=8)
RESTORE = dict(MODEL='hifigan', SPECTROGRAM_ONLY=False, AUGMENT_PITCH=True,
               AUGMENT_LOUDNESS=True, VOCOS_LAYERS=6)
DTYPES = ('fp32', 'f16', 'bf16')
# max-abs relative to the change the block makes
BLOCK_GATE = {'fp32': 6e-6, 'f16': 1.7e-3, 'bf16': 1.2e-2}
# max-abs relative to the peak of the output
HEAD_GATE = {'fp32': 8e-7, 'f16': 7e-5, 'bf16': 5.2e-4}
# max-abs of the batch-32 x 861-frame output (random-init peak 0.118 | 0.99)
FULL_GATE = {('fp32', 'init'): 6.7e-7, ('fp32', 'peak'): 5.7e-6,
             ('f16', 'init'): 2.1e-4, ('f16', 'peak'): 1.8e-3,
             ('bf16', 'init'): 1.8e-3, ('bf16', 'peak'): 1.5e-2}


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


def run_istft(spec, window):
    batch, _, frames = spec.shape
    lib = _lib.lib()
    pairs = torch.view_as_real(spec.to(torch.complex64)).contiguous().cuda()
    window = window.float().contiguous().cuda()
    out = torch.empty(batch, frames * 256, device='cuda')
    ws = torch.empty(lib.pm_istft_workspace_bytes(batch, frames),
                     dtype=torch.uint8, device='cuda')
    _lib.check(lib.pm_istft(
        _lib.ptr(pairs), _lib.ptr(window), _lib.ptr(out), batch, frames,
        ws.data_ptr(), ws.numel(), _lib.stream()))
    return out.cpu()


@pytest.mark.parametrize('frames', [1, 2, 3, 17, 861])
def test_istft_against_irfft_and_fold(device, frames):
    gen = torch.Generator().manual_seed(frames)
    batch = 2
    spec = torch.complex(torch.randn(batch, 513, frames, generator=gen),
                         torch.randn(batch, 513, frames, generator=gen))
    assert spec[:, 0].imag.abs().min() > 0 and spec[:, 512].imag.abs().min() > 0
    # a loaded window that is not Hann (still nonzero where the envelope is)
    window = torch.hann_window(1024) * (
        1 + 0.3 * torch.rand(1024, generator=gen)) + 0.01
    want = oracle.istft(spec, window)
    got = run_istft(spec, window)
    assert got.shape == want.shape
    error = (got - want).abs().max().item() / want.abs().max().item()
    check(error, 6e-7, 'vocos istft rel')


def run_block(x, state, prefix, dtype):
    lib = _lib.lib()
    batch, frames, channels = x.shape
    hidden = state[prefix + 'pwconv1.weight'].shape[0]
    t = {k: state[prefix + k].float().contiguous().cuda() for k in (
        'dwconv.weight', 'dwconv.bias', 'norm.weight', 'norm.bias',
        'pwconv1.weight', 'pwconv1.bias', 'pwconv2.weight', 'pwconv2.bias',
        'gamma')}
    x = x.contiguous().cuda()
    y = torch.empty_like(x)
    code = _lib.DTYPES[dtype]
    ws = torch.empty(lib.pm_convnext_block_workspace_bytes(
        code, channels, hidden), dtype=torch.uint8, device='cuda')
    _lib.check(lib.pm_convnext_block_cl(
        code, _lib.ptr(x), _lib.ptr(y),
        *[_lib.ptr(t[k]) for k in (
            'dwconv.weight', 'dwconv.bias', 'norm.weight', 'norm.bias',
            'pwconv1.weight', 'pwconv1.bias', 'pwconv2.weight',
            'pwconv2.bias', 'gamma')],
        batch, frames, channels, hidden, ws.data_ptr(), ws.numel(),
        _lib.stream()))
    return y.cpu()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('batch,frames', [(1, 5), (3, 130), (5, 67), (2, 1)])
def test_convnext_block(device, dtype, batch, frames):
    state = oracle.random_state_vocos(3, layers=1)
    prefix = 'backbone.convnext.0.'
    # a trained-like block: larger gamma and LayerNorm affine
    gen = torch.Generator().manual_seed(batch * 1000 + frames)
    state[prefix + 'gamma'] = torch.rand(512, generator=gen)
    state[prefix + 'norm.weight'] = 1 + 0.2 * torch.randn(512, generator=gen)
    state[prefix + 'norm.bias'] = 0.1 * torch.randn(512, generator=gen)
    state[prefix + 'dwconv.bias'] = 0.1 * torch.randn(512, generator=gen)
    x = torch.randn(batch, 512, frames, generator=gen)
    want = oracle.convnext_block(x, state, prefix)
    got = run_block(x.transpose(1, 2), state, prefix, dtype).transpose(1, 2)
    # the change the block makes, relative to its own size
    delta = (want - x).abs().max().item()
    error = (got - want).abs().max().item() / delta
    check(error, BLOCK_GATE[dtype], f'vocos block {dtype} rel')


@pytest.mark.parametrize('dtype', DTYPES)
def test_head_exp_clip_and_large_phases(device, dtype):
    gen = torch.Generator().manual_seed(5)
    state = oracle.random_state_vocos(4, layers=0)
    batch, frames = 2, 9
    x = torch.randn(batch, 512, frames, generator=gen)
    weight = torch.randn(1026, 512, generator=gen) * 0.02
    bias = torch.zeros(1026)
    bias[:513] = torch.linspace(-5, 95, 513)     # exp(m) > 100: clipped
    bias[513:] = torch.linspace(-1e3, 1e3, 513)  # |phase| up to 1e3
    state['head.out.weight'], state['head.out.bias'] = weight, bias
    want = oracle.head(x, state)[:, 0]
    lib = _lib.lib()
    code = _lib.DTYPES[dtype]
    xc = x.transpose(1, 2).contiguous().cuda()
    out = torch.empty(batch, frames * 256, device='cuda')
    ws = torch.empty(lib.pm_vocos_head_workspace_bytes(code, batch, frames),
                     dtype=torch.uint8, device='cuda')
    tensors = [t.contiguous().cuda() for t in (
        weight, bias, state['head.istft.window'])]
    _lib.check(lib.pm_vocos_head(
        code, _lib.ptr(xc), *[_lib.ptr(t) for t in tensors], _lib.ptr(out),
        batch, frames, ws.data_ptr(), ws.numel(), _lib.stream()))
    got = out.cpu()
    error = (got - want).abs().max().item() / want.abs().max().item()
    check(error, HEAD_GATE[dtype], f'vocos head {dtype} rel')


def test_vocos_matches_the_reference_golden(device, baseline):
    golden = torch.load(oracle_golden(), weights_only=False)
    state = oracle.random_state_vocos(int(golden['seed']))
    table = torch.randn(109, 256, generator=torch.Generator().manual_seed(
        int(golden['speaker_table_seed'])))
    model = vocos_model(state, device)
    case = 0
    while f'case{case}/mels' in golden:
        mels = golden[f'case{case}/mels']
        g = oracle.global_features(golden[f'case{case}/speakers'], table)
        got = model(mels.to(device), g.to(device)).cpu()
        want = golden[f'case{case}/audio']
        assert got.shape == want.shape
        check((got - want).abs().max().item(), 4.7e-7,
              'vocos golden fp32 abs', case)
        case += 1
    assert case >= 4


def oracle_golden():
    from pathlib import Path
    return Path(__file__).resolve().parent / 'golden' / 'vocos.pt'


@pytest.fixture(scope='module')
def full_size():
    """batch 32 x 861 frames at the baseline config, and the restatement's
    output for 4 of the utterances at the random-init scale"""
    gen = torch.Generator().manual_seed(21)
    mels = torch.randn(32, 80, 861, generator=gen) - 4.
    g = torch.randn(32, 256, 1, generator=gen)
    rows = [0, 7, 19, 31]
    state = oracle.random_state_vocos(21)
    with torch.no_grad():
        want = oracle.vocos(mels[rows], g[rows], state)
    return mels, g, rows, state, want


@pytest.mark.parametrize('scale', ['init', 'peak'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_full_size_every_dtype(device, baseline, full_size, dtype, scale):
    mels, g, rows, state, want = full_size
    if scale == 'peak':
        # the head's log-magnitude bias moves the output to a trained
        # checkpoint's peak (the output is linear in exp(bias) below the clip)
        shift = math.log(0.99 / want.abs().max().item())
        state = dict(state)
        bias = state['head.out.bias'].clone()
        bias[:513] += shift
        state['head.out.bias'] = bias
        want = want * math.exp(shift)
    model = vocos_model(state, device, dtype)
    with torch.no_grad():
        got = model(mels.to(device), g.to(device))
    torch.cuda.synchronize()
    assert got.shape == (32, 1, 861 * 256)
    got = got[rows].cpu()
    assert torch.isfinite(got).all()
    error = (got - want).abs().max().item()
    print(f'{dtype} {scale}: max-abs {error:.3e}, peak '
          f'{want.abs().max().item():.3e}')
    check(error, FULL_GATE[dtype, scale], f'vocos full {dtype} {scale} abs')


@pytest.mark.parametrize('dtype', DTYPES)
def test_rows_are_independent_and_runs_repeat(device, baseline, dtype):
    gen = torch.Generator().manual_seed(8)
    state = oracle.random_state_vocos(8)
    model = vocos_model(state, device, dtype)
    mels = (torch.randn(5, 80, 70, generator=gen) - 4.).to(device)
    g = torch.randn(5, 256, 1, generator=gen).to(device)
    with torch.no_grad():
        batch = model(mels, g).clone()
        again = model(mels, g)
        assert torch.equal(batch, again)
        for b in range(5):
            alone = model(mels[b:b + 1], g[b:b + 1])
            assert torch.equal(alone[0], batch[b]), b


def test_mel_generator_and_baseline_mels(device, baseline, tmp_path):
    import numpy as np
    import scipy.io.wavfile
    promonet_amd.configure(COMPUTE_DTYPE='checkpoint')
    model = promonet_amd.model.MelGenerator().to(device)
    spectrogram = torch.rand(2, 513, 12, device=device)
    speakers = torch.tensor([1, 2], device=device)
    ones = torch.ones(2, device=device)
    with torch.no_grad():
        audio = model(spectrogram, speakers, ones, ones)
        mels = model.prepare_features(spectrogram)
    assert audio.shape == (2, 1, 12 * 256) and mels.shape == (2, 80, 12)
    # MelGenerator = linear_to_mel + prepare_global_features + Vocos
    with torch.no_grad():
        direct = model.model(mels, model.prepare_global_features(
            speakers, ones, ones))
    assert torch.equal(audio, direct)

    mels_api = promonet_amd.baseline.mels
    samples = torch.randn(1, 256 * 20, generator=torch.Generator()
                          .manual_seed(2)) * 0.1
    out = mels_api.from_audio(samples.to(device), speaker=3)
    assert out.shape == (1, 256 * 20), out.shape
    spec = promonet_amd.preprocess.spectrogram.from_audio(samples.to(device))
    assert torch.equal(mels_api.from_features(spec, speaker=3), out)
    wav = tmp_path / 'in.wav'
    scipy.io.wavfile.write(wav, 44100, (samples[0].numpy() * 3e4).astype(
        np.int16))
    target = tmp_path / 'out.wav'
    mels_api.from_file_to_file(wav, target, gpu=0)
    rate, data = scipy.io.wavfile.read(target)
    expected = promonet_amd.load.audio(wav).shape[-1] // 256 * 256
    assert rate == promonet_amd.SAMPLE_RATE and data.shape == (expected,)


def test_cpu_tensors_raise(baseline):
    model = promonet_amd.model.Vocos(80, 256)
    with pytest.raises(RuntimeError, match='GPU'):
        model(torch.zeros(1, 80, 4))
    if torch.cuda.is_available():
        model = model.cuda()
        with pytest.raises(RuntimeError, match='GPU'):
            model(torch.zeros(1, 80, 4))


def test_hifigan_only_dtypes_raise(device, baseline):
    promonet_amd.configure(COMPUTE_DTYPE='f16a2')
    model = promonet_amd.model.Vocos(80, 256).to(device)
    with pytest.raises(ValueError, match='Vocos'):
        model(torch.zeros(1, 80, 4, device=device))
