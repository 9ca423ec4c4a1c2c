"""pm_stft_magnitude_backward and the mel backward kernels past their first
tile, against float64 autograd through the oracle's torch.stft restatement.

Geometry pinned (pm_launch.h, pm_audio.hip): both conv launches tile time in
128 columns and M in 64 rows; the cotangent launch (EPI 3) has 1088 rows = 17
M blocks, rows >= 2 * 513 masked; the overlap-add has 4 M blocks, 17 chunks of
64 channels and a 3-row halo across every 128-column edge; the pad adjoint
folds two mirrors and truncates at Np = (T + 3) * 256; the mel backward
kernels run one workgroup per 256 frames. tests/test_cpu_spectrogram_backward
.py shows that these shapes reject a planted tiling defect.

Metric: e = max|ours - ref64| / max(1, max|ref64|). Ceiling 2e-5 (that of
test_spectrogram_backward); each gate is min(2e-5, 3 x measured). Measured on
an MI355X (PM_RECORD_ERRORS=1), the table MEASURED below: linear 7.3e-7 ..
3.0e-6, log-mel 1.6e-6 .. 3.7e-6, one-hot 2.4e-7, mel backward alone 1.3e-7
(torch's own fp32 autograd of the oracle: 0.3-1.5e-6). The inputs are drawn
so that float32 can meet the ceiling at all (sbo.fp32_floor): the first draw
of the long case holds a Nyquist bin that cancels to |X| = 1.05e-3 under a
weight of 3.4, where the kernel measured 2.9e-5 and torch's fp32 9.4e-6.
"""
import pytest
import torch

import restatement as oracle
import spectrogram_backward_oracle as sbo
from util import check

pytestmark = pytest.mark.gpu

CEILING = sbo.CEILING
# e per kind as measured on an MI355X; a kind that is not listed has not been
# measured and is held to the ceiling alone
MEASURED = {
    'stft_backward:1x32512': 2.36e-06,
    'stft_backward:1x32768': 2.59e-06,
    'stft_backward:1x33024': 2.23e-06,
    'stft_backward:2x31744': 2.40e-06,
    'stft_backward:2x32000': 2.27e-06,
    'stft_backward:2x32261': 2.97e-06,
    'stft_backward:2x385': 8.01e-07,
    'stft_backward:2x511': 7.34e-07,
    'stft_backward:2x512': 1.42e-06,
    'stft_backward:2x640': 1.72e-06,
    'stft_backward:3x76877': 2.64e-06,
    'stft_backward_mel:2x65280': 1.77e-06,
    'stft_backward_mel:2x65536': 1.63e-06,
    'stft_backward_mel:2x65792': 3.14e-06,
    'stft_backward_mel:2x76800': 3.73e-06,
    'stft_backward_one_hot': 2.38e-07,
}


def gate(kind):
    return min(CEILING, 3. * MEASURED.get(kind, CEILING))


def kind_of(prefix, shape):
    return f'{prefix}:{shape[0]}x{shape[1]}'


def spectrogram_graph(device, audio, mels=False, threshold=None):
    import promonet_amd
    leaf = audio.clone().to(device).requires_grad_(True)
    spec = promonet_amd.preprocess.spectrogram.from_audio(
        leaf, mels, threshold)
    assert spec.requires_grad
    return leaf, spec.reshape(audio.shape[0], -1, audio.shape[-1] // sbo.HOP)


def our_gradient(device, audio, weight, mels=False, threshold=None):
    leaf, spec = spectrogram_graph(device, audio, mels, threshold)
    assert spec.shape == weight.shape
    grad, = torch.autograd.grad(spec, leaf, weight.to(device))
    torch.cuda.synchronize()
    return grad[:, 0]


@pytest.mark.parametrize('shape', sbo.LINEAR_SHAPES)
def test_linear(device, shape):
    """Tile edges of both launches, all three factors of the workgroup id
    above 1, the shortest lengths; silence; determinism; one utterance of a
    batch equals its own call."""
    audio, weight = sbo.make_case(*shape)
    reference, _ = sbo.reference_gradient(audio, weight)
    ours = our_gradient(device, audio, weight)
    assert ours.shape == reference.shape == shape
    assert bool(torch.isfinite(ours).all())
    kind = kind_of('stft_backward', shape)
    error = sbo.relative_error(ours, reference)
    print(f'{kind}: e {error:.3e} (grad abs-max '
          f'{reference.abs().max().item():.3e})')
    # a sample no frame reads through a non-zero window has gradient exactly
    # zero in float64: so must ours
    assert sbo.zero_mismatches(ours, reference) == 0
    assert torch.equal(our_gradient(device, audio, weight), ours)
    if shape == sbo.LONG:
        assert bool((ours[sbo.SILENT_UTTERANCE] == 0).all())
        item, first, last = sbo.ZERO_STRETCH
        assert bool((ours[item, first + 1024:last - 1024] == 0).all())
        for item in range(shape[0]):
            alone = our_gradient(
                device, audio[item:item + 1], weight[item:item + 1])
            assert torch.equal(alone[0], ours[item]), item
    check(error, gate(kind), kind)


@pytest.fixture(scope='module')
def long_graphs(device):
    audio, _ = sbo.make_case(*sbo.LONG)
    return sbo.reference_graph(audio), spectrogram_graph(device, audio)


@pytest.mark.parametrize('frame', sbo.ONE_HOT_FRAMES)
@pytest.mark.parametrize('channel', sbo.ONE_HOT_BINS)
def test_one_hot_cotangent(device, long_graphs, channel, frame):
    """One (utterance, bin, frame) of the cotangent: exactly zero outside
    the frame's support in every utterance, float64 inside. Frames 127 | 128
    sit on either side of the tile edge, bin 512 in the last M block."""
    (leaf64, spec64), (leaf, spec) = long_graphs
    item = sbo.ONE_HOT_UTTERANCE
    weight = sbo.one_hot(spec64.shape, item, channel, frame)
    reference, = torch.autograd.grad(
        spec64, leaf64, weight.double(), retain_graph=True)
    ours, = torch.autograd.grad(
        spec, leaf, weight.to(device), retain_graph=True)
    ours, reference = ours[:, 0].cpu(), reference[:, 0]
    support = torch.zeros(sbo.LONG, dtype=torch.bool)
    support[item] = sbo.frame_support(sbo.LONG[1], frame)
    assert bool(torch.isfinite(ours).all())
    assert bool((ours[~support] == 0).all())
    assert bool((reference[support] != 0).all())
    error = sbo.relative_error(ours, reference)
    print(f'one-hot bin {channel} frame {frame}: e {error:.3e} (grad abs-max '
          f'{reference.abs().max().item():.3e})')
    check(error, gate('stft_backward_one_hot'), 'stft_backward_one_hot')


@pytest.mark.parametrize('shape', sbo.MEL_SHAPES)
def test_log_mel(device, shape):
    """from_audio(mels=True) differentiated: the STFT backward behind both
    mel backward kernels, at 255 | 256 | 257 frames (the second 256-frame
    workgroup) and 300, the clamp active on part of the tensor."""
    audio, weight = sbo.make_case(*shape, channels=80)
    _, unclamped = sbo.reference_gradient(audio, weight, True)
    threshold, margin = sbo.clamp_threshold(unclamped)
    assert margin > 2e-5            # fp32 log-mel is within 1e-5 of float64
    assert (unclamped < threshold).any() and (unclamped > threshold).any()
    reference, mel = sbo.reference_gradient(audio, weight, True, threshold)
    assert (mel == threshold).any() and (mel > threshold).any()
    ours = our_gradient(device, audio, weight, True, threshold)
    assert bool(torch.isfinite(ours).all())
    kind = kind_of('stft_backward_mel', shape)
    error = sbo.relative_error(ours, reference)
    print(f'{kind}: threshold {threshold:.6f} +- {margin:.1e}, e {error:.3e} '
          f'(grad abs-max {reference.abs().max().item():.3e})')
    assert torch.equal(
        our_gradient(device, audio, weight, True, threshold), ours)
    check(error, gate(kind), kind)


@pytest.mark.parametrize('frames', [256, 257])
def test_linear_to_mel_alone(device, frames):
    """blockIdx.x == 1 in pm_mel_backward_rows_kernel and _cols_kernel; the
    gate is the one test_spectrogram_backward holds the mel-alone case to."""
    import promonet_amd
    gen = torch.Generator().manual_seed(40 + frames)
    spec = torch.rand(2, 513, frames, generator=gen) + .01
    weight = torch.randn(2, 80, frames, generator=gen)
    # (log-mel of this input spans -6.3 .. -3.1, median -3.74: the -2. of
    # test_spectrogram_backward would clamp every element)
    threshold, margin = sbo.clamp_threshold(
        oracle.linear_to_mel(spec.double()), -3.9, -3.6)
    assert margin > 2e-5
    leaf64 = spec.double().requires_grad_(True)
    mel = oracle.linear_to_mel(leaf64, threshold=threshold)
    assert (mel == threshold).any() and (mel > threshold).any()
    reference, = torch.autograd.grad(mel, leaf64, weight.double())
    leaf = spec.to(device).requires_grad_(True)
    out = promonet_amd.preprocess.spectrogram.linear_to_mel(leaf, threshold)
    ours, = torch.autograd.grad(out, leaf, weight.to(device))
    scale = max(1., reference.abs().max().item())
    error = (ours.double().cpu() - reference).abs().max().item() / scale
    print(f'mel backward alone, {frames} frames: {error:.3e}')
    # the second workgroup's frames, on their own
    if frames > 256:
        tail = (ours.double().cpu() - reference)[..., 256:].abs().max().item()
        assert 0 < tail < 1e-4 * scale
    check(error, 1e-4, f'mel_backward_alone:{frames}')


def carve(device, size):
    """`size` bytes at a 256-byte-aligned address inside a larger buffer of
    0xA5, 4096 guard bytes or more on both sides."""
    whole = torch.full(
        (size + 2 * 4096 + 256,), 0xA5, dtype=torch.uint8, device=device)
    first = 4096 + (-(whole.data_ptr() + 4096)) % 256
    assert (whole.data_ptr() + first) % 256 == 0
    return whole, first


def guards_intact(whole, first, size):
    return bool((whole[:first] == 0xA5).all()) and \
        bool((whole[first + size:] == 0xA5).all())


def test_c_abi_scratch_and_guards(device):
    """pm_stft_magnitude_backward with exactly the scratch it asks for and
    an output of N % 256 != 0 samples, both inside guarded buffers: nothing
    outside is written, the result is the autograd path's bit for bit; one
    byte less is refused before anything is written."""
    from promonet_amd import _lib
    lib = _lib.lib()
    shape = (2, sbo.HOP * 130 + 77)
    audio, weight = sbo.make_case(*shape)
    want = our_gradient(device, audio, weight)
    flat = audio[:, 0].contiguous().to(device)
    grad = weight.contiguous().to(device)
    size = lib.pm_stft_backward_scratch_bytes(*shape)
    assert size > 0
    scratch, scratch_at = carve(device, size)
    out_bytes = 4 * shape[0] * shape[1]
    assert shape[1] % 256
    result, result_at = carve(device, out_bytes)

    def call(scratch_bytes):
        _lib.check(lib.pm_stft_magnitude_backward(
            _lib.ptr(flat), _lib.ptr(grad), result.data_ptr() + result_at,
            shape[0], shape[1], scratch.data_ptr() + scratch_at,
            scratch_bytes, _lib.stream()))
        torch.cuda.synchronize()

    with pytest.raises(RuntimeError):
        call(size - 1)
    torch.cuda.synchronize()
    assert bool((result == 0xA5).all()) and bool((scratch == 0xA5).all())
    call(size)
    assert guards_intact(scratch, scratch_at, size)
    assert guards_intact(result, result_at, out_bytes)
    got = result[result_at:result_at + out_bytes].view(torch.float32)
    assert torch.equal(got.reshape(shape), want)
