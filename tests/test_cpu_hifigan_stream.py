"""CPU: HiFi-GAN streaming by overlap-save - the context
formula against a float64 perturbation check, the schedule, the streaming
oracle against the full forward, and the defects the comparison of the GPU
tests has to catch."""
import ctypes
import random

import pytest
import torch

import hifigan_stream_oracle as stream_oracle
import restatement as oracle
from promonet_amd import _lib
from promonet_amd.model.hifigan import hifigan_context, stream_schedule

DEFAULT = ((8, 8, 2, 2), (16, 16, 4, 4), (3, 7, 11), ((1, 3, 5),) * 3)
CONFIGS = {
    'default': DEFAULT,
    'two_stages': ((4, 4), (8, 8), (3, 5), ((1, 2),) * 2),
    'one_block': ((2, 4, 2), (4, 8, 4), (7,), ((1, 3, 5),))}

# float64 rounding of sums of positive terms below 1: the window and the full
# forward may add in another order
ROUNDING = 1e-12

SIZES = (1, 2, 5, 13, 14, 27, 40)
LONGEST = 45
LEFT = 13
LOOKAHEADS = (0, 1, 12, 13)


def sequences(count=600, seed=0):
    """Chunk sequences over SIZES with at most LONGEST frames: a fixed few
    that every edge shows in, then sampled ones (all of them are far too
    many: there are 2^44 with ones alone)"""
    fixed = [[40], [5] * 9, [1] * 45, [13, 13, 13], [14, 14, 14],
             [27, 13, 5], [40, 5], [5, 40], [1, 40, 2, 2], [2, 1, 13, 14, 5],
             [13, 27, 5], [14, 27, 2, 2], [1], [2], [13], [14], [27, 14]]
    fixed = [s for s in fixed if all(c in SIZES for c in s)]
    rng = random.Random(seed)
    out = {tuple(s) for s in fixed}
    while len(out) < count:
        chunks, target = [], rng.randint(1, LONGEST)
        while True:
            fits = [c for c in SIZES if sum(chunks) + c <= target]
            if not fits:
                break
            chunks.append(rng.choice(fits))
        if chunks:
            out.add(tuple(chunks))
    return sorted(out)


@pytest.fixture
def configured(monkeypatch):
    """restatement.hifigan_forward reads the Blocks' shape from its module"""
    def configure(name):
        rates, kernels, res_kernels, res_dilations = CONFIGS[name]
        monkeypatch.setattr(oracle, 'RESBLOCK_KERNEL_SIZES', res_kernels)
        monkeypatch.setattr(oracle, 'RESBLOCK_DILATION_SIZES', res_dilations)
        return CONFIGS[name]
    return configure


###############################################################################
# Context
###############################################################################


def test_context_at_the_defaults():
    assert hifigan_context(*DEFAULT) == (13, 13)
    import promonet_amd
    assert hifigan_context(
        promonet_amd.HIFIGAN_UPSAMPLE_RATES,
        promonet_amd.HIFIGAN_UPSAMPLE_KERNEL_SIZES,
        promonet_amd.HIFIGAN_RESBLOCK_KERNEL_SIZES,
        promonet_amd.HIFIGAN_RESBLOCK_DILATION_SIZES) == (13, 13)


def test_context_refuses_a_fractional_padding():
    with pytest.raises(ValueError):
        hifigan_context((2, 2), (7, 4), (3,), ((1,),))


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_context_is_tight(configured, name):
    """With outer-tap weights and positive inputs the window [first - L,
    last + R) reproduces frames [first, last) of the full forward with the
    derived (L, R), and one frame less on either side changes a run of
    samples at that edge."""
    config = configured(name)
    rates = config[0]
    hop = 1
    for r in rates:
        hop *= r
    left, right = hifigan_context(*config)
    state = stream_oracle.outer_tap_state(*config)
    first, last = left + 12, left + 20
    frames = last + right + 12
    features = stream_oracle.positive_inputs(1, 4, frames)
    forward = stream_oracle.window_forward(features, state)
    want = forward(0, frames)[..., first * hop:last * hop]
    assert 0 < want.min() and want.max() < 1

    def window(l, r):
        return forward(first - l, last + r)[..., l * hop:(l + last - first) * hop]

    assert (window(left, right) - want).abs().max().item() <= ROUNDING
    # (a sample CHANGES when it moves by more than 1e-15 of its value - a few
    # float64 roundings: the longest path into the outermost frame, through
    # every conv of the k 11 Blocks, carries 3e-15 of a sample's value)
    short = (window(left - 1, right) - want).abs() > 1e-15 * want
    changed = short.nonzero()[:, -1]
    assert 0 < len(changed) <= hop
    assert changed.tolist() == list(range(len(changed)))
    short = (window(left, right - 1) - want).abs() > 1e-15 * want
    changed = short.nonzero()[:, -1]
    assert 0 < len(changed) <= hop
    assert changed.tolist() == list(range(
        want.shape[-1] - len(changed), want.shape[-1]))
    if name == 'default':
        print(f'context {left}, {right}: one frame less changes {len(changed)} '
              'samples at the edge')
        # (the interval arithmetic, sample by sample: samples 70 ... 255 of a
        # frame read the 13th frame after it)
        assert len(changed) == 186


def default_config():
    rates, kernels, res_kernels, res_dilations = DEFAULT
    config = _lib.HifiganConfig()
    config.num_features, config.global_channels = 113, 258
    config.initial_channels, config.num_stages = 512, len(rates)
    for i, (r, k) in enumerate(zip(rates, kernels)):
        config.upsample_rates[i], config.upsample_kernel_sizes[i] = r, k
    config.num_resblocks = len(res_kernels)
    config.num_dilations = len(res_dilations[0])
    for j, k in enumerate(res_kernels):
        config.resblock_kernel_sizes[j] = k
        for n, d in enumerate(res_dilations[j]):
            config.resblock_dilations[j][n] = d
    config.compute_dtype = _lib.PM_F16
    return config


def test_c_context_agrees():
    """pm_hifigan_context on an engine of the default configuration (created
    on the host: no weights, no GPU call)"""
    lib = _lib.lib()
    handle = ctypes.c_void_p()
    assert lib.pm_hifigan_create(
        ctypes.byref(default_config()), ctypes.byref(handle)) == 0
    try:
        left, right = ctypes.c_int(), ctypes.c_int()
        assert lib.pm_hifigan_context(
            handle, ctypes.byref(left), ctypes.byref(right)) == 0
        assert (left.value, right.value) == (13, 13)
        assert lib.pm_hifigan_context(handle, None, None) == _lib.PM_EINVAL

        # the argument checks of pm_hifigan_stream mirror the schedule (they
        # answer before the first HIP call)
        def step(chunk, prev, keep, first, count):
            fake = ctypes.c_void_p(4096)
            return lib.pm_hifigan_stream(
                handle, fake, 1, chunk, fake, prev, keep,
                ctypes.c_void_p(1 << 30), fake, 1, first, count, fake, 1,
                fake, 1 << 40, None)
        for bad in [(8, 4, 5, 0, 1),        # keep > prev_frames
                    (8, 40, 27, 0, 1),      # keep > left + right
                    (8, 26, 26, 30, 5),     # emitted frames past the window
                    (0, 0, 0, 0, 0),        # empty window
                    (-1, 0, 0, 0, 0), (8, 8, 8, -1, 1)]:
            assert step(*bad) == _lib.PM_EINVAL, bad
        assert b'alias' not in lib.pm_last_error()
        fake = ctypes.c_void_p(4096)
        assert lib.pm_hifigan_stream(
            handle, fake, 1, 8, fake, 8, 8, fake, fake, 1, 0, 1, fake, 1,
            fake, 1 << 40, None) == _lib.PM_EINVAL
        assert b'alias' in lib.pm_last_error()
        assert lib.pm_hifigan_stream_workspace_bytes(handle, 0, 8) == 0
        assert lib.pm_hifigan_stream_workspace_bytes(None, 1, 8) == 0
    finally:
        lib.pm_hifigan_destroy(handle)


###############################################################################
# Schedule
###############################################################################


def run_schedule(chunks, lookahead, left=LEFT):
    """The package's schedule over `chunks` and the final step, as absolute
    (window_first, window_last, emit_first, emit_last, keep, pushed)"""
    seen, steps = 0, []
    for chunk in list(chunks) + [None]:
        final = chunk is None
        keep, first, count, after = stream_schedule(
            seen, 0 if final else chunk, left, lookahead, final)
        start = seen - keep
        steps.append((start, after, start + first, start + first + count,
                      keep, seen))
        seen = after
    return steps


@pytest.mark.parametrize('lookahead', LOOKAHEADS)
def test_schedule_tiles_the_utterance(lookahead):
    cases = sequences()
    assert len(cases) >= 500
    for chunks in cases:
        total, position = sum(chunks), 0
        steps = run_schedule(chunks, lookahead)
        for start, end, first, last, keep, pushed in steps:
            assert first == position and last >= first, chunks
            position = last
            assert 0 <= keep <= pushed, chunks
            assert start >= 0 and end <= total
            if last > first:
                assert start == max(0, first - LEFT), chunks
                assert first >= start and last <= end
        assert position == total, chunks
        # and it is the oracle's, step for step
        assert [s[:4] for s in steps] == [
            r[:4] for r in stream_oracle.ranges(chunks, LEFT, lookahead)]


def test_schedule_refuses_nonsense():
    with pytest.raises(ValueError):
        stream_schedule(-1, 4, 13, 13)
    with pytest.raises(ValueError):
        stream_schedule(4, 4, 13, 13, final=True)


###############################################################################
# Stream oracle
###############################################################################


@pytest.fixture(scope='module')
def tight():
    """The default configuration with the outer-tap state, 16 channels in
    front: (features, state, forward(first, last))"""
    state = stream_oracle.outer_tap_state(*DEFAULT)
    features = stream_oracle.positive_inputs(2, 4, LONGEST, seed=5)
    return features, state


def test_stream_oracle_equals_the_full_forward(tight):
    features, state = tight
    forward = stream_oracle.window_forward(features, state)
    for chunks in sequences():
        total = sum(chunks)
        got = stream_oracle.stream(chunks, LEFT, 13, forward, 256)
        assert len(got) == len(chunks) + 1
        assert stream_oracle.close(got, forward(0, total), ROUNDING), chunks


@pytest.mark.parametrize('lookahead', [0, 1, 12])
def test_stream_oracle_reduced_lookahead(tight, lookahead):
    """What a push emits is the forward of the utterance that ends where the
    stream has got to, on those frames; finish() is the full forward's tail"""
    features, state = tight
    forward = stream_oracle.window_forward(features, state)
    for chunks in sequences():
        got = stream_oracle.stream(chunks, LEFT, lookahead, forward, 256)
        seen, position = 0, 0
        for chunk, audio in zip(list(chunks) + [0], got):
            seen += chunk
            emitted = audio.shape[-1]
            want = forward(0, seen)[..., position:position + emitted]
            assert want.shape == audio.shape
            if emitted:
                assert (audio - want).abs().max().item() <= ROUNDING, chunks
            position += emitted
        assert position == seen * 256


@pytest.mark.parametrize('defect', stream_oracle.DEFECTS)
def test_planted_defects_are_rejected(tight, defect):
    """The comparison of the GPU tests - the concatenated audio against one
    forward, shape and bits - must reject each of them (float64 here: every
    honest difference is rounding, every defect is not)"""
    features, state = tight
    forward = stream_oracle.window_forward(features, state)
    chunks = [8] * 5 + [5]
    full = forward(0, LONGEST)
    honest = stream_oracle.stream(chunks, LEFT, 13, forward, 256)
    assert stream_oracle.close(honest, full, ROUNDING)
    broken = stream_oracle.stream(chunks, LEFT, 13, forward, 256, defect)
    assert not stream_oracle.close(broken, full, ROUNDING)
    assert not stream_oracle.same(broken, full)
    joined = torch.cat(broken, dim=-1)
    if defect == 'no_finish':
        assert joined.shape[-1] == (LONGEST - 13) * 256
    elif joined.shape == full.shape:
        assert ((joined - full).abs() > ROUNDING * full).any()


def test_fargan_generator_points_to_its_own_stream():
    import promonet_amd
    promonet_amd.configure(MODEL='fargan')
    try:
        model = promonet_amd.model.Generator()
    finally:
        promonet_amd.configure(MODEL='hifigan')
    with pytest.raises(ValueError, match='FARGAN.stream'):
        model.packed_stream()
    with pytest.raises(ValueError, match='FARGAN.stream'):
        model.open_stream(torch.zeros(1), torch.ones(1), torch.ones(1))


def test_a_cpu_model_does_not_stream():
    import promonet_amd
    model = promonet_amd.model.HiFiGAN(113, 258)
    with pytest.raises(RuntimeError, match='AMD GPU'):
        model.open_stream(torch.zeros(1, 258, 1), 1)
