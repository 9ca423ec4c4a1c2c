"""The checks of tests/test_gpu_spectrogram_backward.py can fail: a float64
restatement of the kernels' algorithm (tests/spectrogram_backward_oracle.py)
equals float64 autograd, and with a tiling or mirror defect planted it misses
the GPU file's gate or one of its exact-zero assertions - at the GPU file's
shapes, not at the shapes the suite ran before. No GPU."""
import pytest
import torch

import spectrogram_backward_oracle as sbo

GATE = sbo.CEILING  # of test_spectrogram_backward and of the GPU file


@pytest.fixture(scope='module')
def cases():
    """Per shape: inputs, the float64 autograd gradient, the restatement."""
    out = {}
    for shape in sbo.LINEAR_SHAPES + sbo.OLD_SHAPES:
        audio, weight = sbo.make_case(*shape)
        reference, _ = sbo.reference_gradient(audio, weight)
        out[shape] = (audio, weight, reference,
                      sbo.restated_gradient(audio, weight))
    return out


def caught(planted, reference):
    """What the GPU file asserts of a gradient, as a list of misses."""
    misses = []
    if not bool(torch.isfinite(planted).all()):
        misses.append('finite')
    if sbo.relative_error(planted, reference) >= GATE:
        misses.append('gate')
    if sbo.zero_mismatches(planted, reference):
        misses.append('zero')
    return misses


@pytest.mark.parametrize('shape', sbo.LINEAR_SHAPES + sbo.OLD_SHAPES)
def test_restatement_is_the_gradient(cases, shape):
    audio, weight, reference, restated = cases[shape]
    assert restated.shape == reference.shape == shape
    assert sbo.relative_error(restated, reference) < 1e-10
    # an independent framing: explicit float64 DFT instead of torch.stft
    assert sbo.relative_error(
        restated, sbo.reference_gradient_dft(audio, weight)) < 1e-10
    assert caught(restated, reference) == []


@pytest.mark.parametrize('shape', sbo.LINEAR_SHAPES)
def test_ceiling_can_be_asked_of_float32(cases, shape):
    """Where a bin cancels to |X| ~ 1e-3 under a large weight, the forward's
    float32 rounding alone exceeds the ceiling (the first draw of the long
    case: floor 8.5e-5, torch's own fp32 autograd 9.4e-6 off float64 where it
    is 0.3-1.5e-6 otherwise, the kernel 2.9e-5): make_case draws again."""
    audio, weight = cases[shape][:2]
    assert sbo.fp32_floor(audio, weight) <= sbo.CEILING
    if shape == sbo.LONG:
        first = sbo.draw_case(*shape, sbo.BINS, 0)
        assert sbo.fp32_floor(*first) > sbo.CEILING
        assert not torch.equal(first[0], audio)


def test_silence_is_exactly_zero_in_float64(cases):
    """The premise of the GPU file's silence assertions."""
    audio, _, reference, restated = cases[sbo.LONG]
    item, first, last = sbo.ZERO_STRETCH
    for gradient in (reference, restated):
        assert bool((gradient[sbo.SILENT_UTTERANCE] == 0).all())
        assert bool((gradient[item, first + 1024:last - 1024] == 0).all())
        assert bool((gradient[item, first - 1024:first] != 0).all())
    assert bool((audio[item, 0, first:last] == 0).all())


# where each defect must show (and, for the tiling ones, only past one tile)
EXPECTED = {
    'halo_dropped': {(2, 256 * 126 + 5), (1, 256 * 127),
                     (1, 256 * 128), (1, 256 * 129), sbo.LONG},
    'wrong_tile': {(1, 256 * 129), sbo.LONG},
    # (at 256 * 126 + 5 the five samples past Np weigh hann(1..4) < 2e-4)
    'right_mirror_untruncated': {(2, 385), (2, 511), (2, 640), sbo.LONG},
    'right_mirror_at_last': set(sbo.LINEAR_SHAPES),
    'padding_rows_live': {shape for shape in sbo.LINEAR_SHAPES if shape[0] > 1},
}


@pytest.mark.parametrize('defect', sorted(EXPECTED))
def test_planted_defect_is_rejected(cases, defect):
    rejected = set()
    for shape in sbo.LINEAR_SHAPES:
        audio, weight, reference, _ = cases[shape]
        planted = sbo.restated_gradient(audio, weight, defect)
        if caught(planted, reference):
            rejected.add(shape)
    assert rejected == EXPECTED[defect], sorted(rejected)


def test_left_mirror_at_pad_cannot_be_seen():
    """`i == pad` of the left mirror adds padded sample 0, which only frame 0
    reads, through hann(0) == 0: its gradient is exactly zero. The defect is
    invisible to ANY test of the gradient - recorded here so that nobody
    looks for a shape that shows it."""
    assert torch.hann_window(sbo.NFFT, dtype=torch.float64)[0] == 0
    for shape in ((2, 385), (2, 640), (1, 256 * 127)):
        audio, weight = sbo.make_case(*shape)
        assert torch.equal(
            sbo.restated_gradient(audio, weight, 'left_mirror_skips_pad'),
            sbo.restated_gradient(audio, weight))


@pytest.mark.parametrize('defect', sbo.TILE_DEFECTS + (
    'right_mirror_untruncated',))
def test_old_shapes_did_not_see_it(cases, defect):
    """T = 24, 9, 31 fit one 128-column tile, and their right mirror never
    meets the truncation with a following utterance to read from: the gap."""
    for shape in sbo.OLD_SHAPES:
        audio, weight, _, restated = cases[shape]
        assert torch.equal(
            sbo.restated_gradient(audio, weight, defect), restated)


@pytest.fixture(scope='module')
def long_graph():
    audio, _ = sbo.make_case(*sbo.LONG)
    return (audio,) + sbo.reference_graph(audio)


@pytest.mark.parametrize('frame', sbo.ONE_HOT_FRAMES)
@pytest.mark.parametrize('channel', sbo.ONE_HOT_BINS)
def test_support_is_the_nonzero_pattern(long_graph, channel, frame):
    audio, leaf, spec = long_graph
    item = sbo.ONE_HOT_UTTERANCE
    weight = sbo.one_hot(spec.shape, item, channel, frame, torch.float64)
    grad, = torch.autograd.grad(spec, leaf, weight, retain_graph=True)
    support = torch.zeros(sbo.LONG, dtype=torch.bool)
    support[item] = sbo.frame_support(sbo.LONG[1], frame)
    assert torch.equal(grad[:, 0] != 0, support)
    restated = sbo.restated_gradient(audio, weight)
    assert torch.equal(restated != 0, support)
    assert sbo.relative_error(restated, grad[:, 0]) < 1e-10


def test_support_folds_at_both_ends():
    """One frame over 385 samples: both mirrors lie on the body."""
    for samples, frame in ((385, 0), (640, 0), (640, 1)):
        audio, _ = sbo.make_case(2, samples)
        leaf, spec = sbo.reference_graph(audio)
        weight = sbo.one_hot(spec.shape, 1, 7, frame, torch.float64)
        grad, = torch.autograd.grad(spec, leaf, weight)
        support = torch.zeros(2, samples, dtype=torch.bool)
        support[1] = sbo.frame_support(samples, frame)
        assert torch.equal(grad[:, 0] != 0, support)


@pytest.mark.parametrize('defect,channel,frame,miss', [
    ('halo_dropped', 256, 127, 'gate'),
    ('wrong_tile', 1, 128, 'gate'),
    ('padding_rows_live', 0, 0, 'zero'),
    ('padding_rows_live', 1, 299, 'zero')])
def test_one_hot_rejects(long_graph, defect, channel, frame, miss):
    """The one-hot cotangents catch the tiling defects at the frames beside
    the tile edge, and a live padding row through the exact zeros of the
    utterance before."""
    audio, leaf, spec = long_graph
    weight = sbo.one_hot(
        spec.shape, sbo.ONE_HOT_UTTERANCE, channel, frame, torch.float64)
    grad, = torch.autograd.grad(spec, leaf, weight, retain_graph=True)
    planted = sbo.restated_gradient(audio, weight, defect)
    assert miss in caught(planted, grad[:, 0])
