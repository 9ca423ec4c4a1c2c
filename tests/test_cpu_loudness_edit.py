"""The loudness-editing oracle on the host: the restatement of `limit` and
`shift` against the golden the reference wrote, the literal loop against its
fp32 form, the chunked model of the device algorithm against both, the facts
the kernel rests on, and the argument checks of
pm_limit and pm_loudness_shift. No GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

from promonet_amd import _lib
from promonet_amd.preprocess import loudness
import loudness_edit_oracle as oracle
from conftest import GOLDEN

CHUNK, TILE = loudness.limit_tile()


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN / 'loudness_edit.pt', weights_only=True)


@pytest.fixture(scope='module')
def classes():
    return oracle.inputs(CHUNK, TILE)


@pytest.fixture(scope='module')
def sequential(classes):
    """name -> (output, gain) of the fp32 form, each class one row"""
    return {name: oracle.limit_rows(x) for name, x in classes.items()}


def test_tile_geometry():
    assert CHUNK >= 1 and TILE >= 2 * CHUNK and TILE % CHUNK == 0
    # the test inputs stay short enough for the literal oracle
    assert 2 * TILE + 256 <= 6011


def test_oracle_equals_the_golden(golden):
    audio = golden['limit/audio']
    cases = [key for key in golden if key.endswith('/parameters')]
    assert len(cases) == 3
    for key in cases:
        delay, attack, release, threshold = golden[key].tolist()
        want = golden[key.replace('parameters', 'output')]
        parameters = dict(delay=int(delay), attack_coef=attack,
                          release_coef=release, threshold=threshold)
        got, _ = oracle.limit_literal(audio, **parameters)
        assert torch.equal(got, want), key
        assert torch.equal(oracle.limit_rows(audio, **parameters)[0], want)
    for index in range(3):
        key = f'shift/case{index}/'
        got = oracle.shift64(golden[key + 'audio'], golden[key + 'value'])
        want = golden[key + 'output']
        assert ((got - want).abs() <= 1e-12 * want.abs()).all(), key
    assert torch.equal(
        oracle.shift64(golden['shift/scalar/audio'],
                       golden['shift/scalar/value'].item()),
        golden['shift/scalar/output'])


def test_literal_and_fp32_forms_are_equal(classes, sequential):
    for name, x in classes.items():
        out, gain = oracle.literal(name, None, CHUNK, TILE)
        assert out.dtype == torch.float32 and out.shape == x.shape
        assert torch.equal(out, sequential[name][0]), name
        assert torch.equal(gain[None], sequential[name][1]), name
    # rows of a batch are independent
    pair = torch.cat([classes['bursts'], classes['edges']])
    out, gain = oracle.limit_rows(pair)
    assert torch.equal(out[1:], sequential['edges'][0])
    assert torch.equal(gain[:1], sequential['bursts'][1])


@pytest.mark.parametrize('L', [1, 7, 64, 256])
def test_chunked_equals_sequential(classes, sequential, L):
    for name, x in classes.items():
        out, gain, serial = oracle.chunked(x, L)
        assert torch.equal(out, sequential[name][0]), name
        assert torch.equal(gain[None], sequential[name][1]), name
        if name == 'quiet':
            assert serial == 0          # fact 2: no serial work at all
    parameters = dict(delay=7, attack_coef=.5, release_coef=.99, threshold=.5)
    out, gain, _ = oracle.chunked(classes['bursts'], L, **parameters)
    want = oracle.limit_rows(classes['bursts'], **parameters)
    assert torch.equal(out, want[0]) and torch.equal(gain[None], want[1])


def test_quiet_input_comes_back(classes, sequential):
    assert classes['quiet'].abs().max() < .99
    out, gain = sequential['quiet']
    assert torch.equal(out, classes['quiet'])
    assert (gain == 1).all()            # the fixed point 1.0f stays


def test_the_gain_settles_at_its_other_fixed_point(classes, sequential):
    delay, a, b, r, th = oracle.coefficients()
    assert np.float32(1) * a + b == np.float32(1)
    assert oracle.REST * a + b == oracle.REST and oracle.REST != 1
    assert float(oracle.REST) == 1 - 4 * 2. ** -24
    # the envelope of the settle class: above th from sample 100 on, for as
    # long as 1.0 r^k stays above it
    x = classes['settle'][0].numpy()
    e, last = np.float32(0), None
    for n in range(len(x)):
        e = max(abs(x[n]), e * r)
        if e > th:
            last = n
    assert 100 <= last <= 100 + 21
    gain = sequential['settle'][1][0].numpy()
    assert (gain[:100] == 1).all() and gain[100] < 1
    assert (gain[last + 200:] == oracle.REST).all()
    assert len(gain) > last + 400
    # from then on the output is the input times 1 - 4 ulp, for ever
    out = sequential['settle'][0][0].numpy()
    lag = delay - 1
    assert (out[last + 200:] == x[last + 200:] * oracle.REST).all()
    assert (out[:100 - lag] == x[:100 - lag]).all()


def test_the_limiter_does_not_hold_the_output_under_one(classes, sequential):
    assert sequential['bursts'][0].abs().max() > 1


def limit_call(library, **overrides):
    """pm_limit with valid sizes and fake, never dereferenced, pointers"""
    a = dict(x=0x10000, lengths=None, out=0x80000, gain=None, rows=2,
             samples=1000, x_stride=1000, out_stride=1000, delay=40,
             attack=.9, complement=.1, release=.9995, threshold=.99,
             workspace=0x1000, workspace_bytes=256)
    a.update(overrides)
    return library.pm_limit(
        a['x'], a['lengths'], a['out'], a['gain'], a['rows'], a['samples'],
        a['x_stride'], a['out_stride'], a['delay'], a['attack'],
        a['complement'], a['release'], a['threshold'], a['workspace'],
        a['workspace_bytes'], None)


def shift_call(library, **overrides):
    a = dict(x=0x10000, db=0x1000, lengths=None, frame_lengths=None,
             out=0x80000, rows=2, samples=1000, x_stride=1000, frames=9,
             db_stride=9, out_stride=1000)
    a.update(overrides)
    return library.pm_loudness_shift(
        a['x'], a['db'], a['lengths'], a['frame_lengths'], a['out'],
        a['rows'], a['samples'], a['x_stride'], a['frames'], a['db_stride'],
        a['out_stride'], None)


def test_signatures_and_argument_checks():
    for name, count in (('pm_limit', 16), ('pm_loudness_shift', 12),
                        ('pm_limit_tile', 2), ('pm_limit_workspace_bytes', 1)):
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == count, name
    assert _lib.SIGNATURES['pm_limit'][0] is ctypes.c_int
    assert _lib.SIGNATURES['pm_limit_workspace_bytes'][0] is ctypes.c_size_t
    library = _lib.lib()
    assert library.pm_limit_workspace_bytes(0) == 0
    assert library.pm_limit_workspace_bytes(2) == 256
    for overrides, code, message in [
            (dict(rows=-1), _lib.PM_EINVAL, 'negative'),
            (dict(samples=-1), _lib.PM_EINVAL, 'negative'),
            (dict(delay=0), _lib.PM_EINVAL, 'delay'),
            (dict(delay=-3), _lib.PM_EINVAL, 'delay'),
            (dict(attack=0.), _lib.PM_EINVAL, '(0, 1)'),
            (dict(attack=1.), _lib.PM_EINVAL, '(0, 1)'),
            (dict(complement=0.), _lib.PM_EINVAL, '(0, 1)'),
            (dict(release=1.5), _lib.PM_EINVAL, '(0, 1)'),
            (dict(release=-.5), _lib.PM_EINVAL, '(0, 1)'),
            (dict(threshold=0.), _lib.PM_EINVAL, 'threshold'),
            (dict(threshold=float('inf')), _lib.PM_EINVAL, 'threshold'),
            (dict(x_stride=999), _lib.PM_EINVAL, 'stride'),
            (dict(out_stride=999), _lib.PM_EINVAL, 'stride'),
            (dict(x=None), _lib.PM_EINVAL, 'null'),
            (dict(out=None), _lib.PM_EINVAL, 'null'),
            (dict(workspace=None), _lib.PM_EINVAL, 'null'),
            (dict(out=0x10000), _lib.PM_EINVAL, 'alias'),
            # the last float of x is the first of out
            (dict(out=0x10000 + 4 * 1999), _lib.PM_EINVAL, 'alias'),
            (dict(workspace_bytes=255), _lib.PM_ENOMEM, 'workspace')]:
        got = limit_call(library, **overrides)
        assert got == code, overrides
        assert message in library.pm_last_error().decode(), overrides
        with pytest.raises(_lib.LibraryError):
            _lib.check(got)
    # nothing to do is not an error, and launches nothing
    assert limit_call(library, rows=0) == 0
    assert limit_call(library, samples=0, x_stride=0, out_stride=0) == 0
    for overrides, message in [
            (dict(rows=-1), 'negative'), (dict(samples=-1), 'negative'),
            (dict(frames=0), 'frames'), (dict(frames=-2), 'frames'),
            (dict(x_stride=999), 'stride'), (dict(out_stride=999), 'stride'),
            (dict(db_stride=8), 'stride'), (dict(rows=65536), 'rows'),
            (dict(x=None), 'null'), (dict(db=None), 'null'),
            (dict(out=None), 'null')]:
        got = shift_call(library, **overrides)
        assert got == _lib.PM_EINVAL, overrides
        assert message in library.pm_last_error().decode(), overrides
    assert shift_call(library, rows=0) == 0
    assert shift_call(library, samples=0, x_stride=0, out_stride=0) == 0


def test_the_product_refuses_host_tensors():
    x = torch.zeros(1, 100)
    for call in (lambda: loudness.limit(x), lambda: loudness.shift(x, 3.),
                 lambda: loudness.scale(x, torch.zeros(1, 1))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def shift_fp32_on_the_host(audio, value):
    """The reference's own path (loudness.py:179-193) in fp32 on the CPU"""
    gain = 2 ** (value / 10)
    gain = torch.nn.functional.interpolate(
        gain[None], size=audio.shape[1], mode='linear',
        align_corners=False)[0]
    return gain * audio


SHIFT_SHAPES = ((1, 300), (2, 513), (9, 2321), (40, 10240 + 17))


def host_shift_units():
    """The largest relative error, in units of 2^-24, of torch's own fp32 path
    on the CPU at (9, 2 321) with the inputs the device test uses: 4 x this
    caps the device test's gate. (At (40, 10 257) the same path is 139 units
    off: its source index is a float, and that error is no yardstick.)"""
    audio, value = oracle.shift_inputs(9, 2321)
    return oracle.relative_units(
        shift_fp32_on_the_host(audio, value), oracle.shift64(audio, value))


def test_the_closed_form_is_torchs_interpolation():
    for frames, samples in SHIFT_SHAPES[1:]:
        audio, value = oracle.shift_inputs(frames, samples)
        want = shift_fp32_on_the_host(audio.double(), value.double())
        got = oracle.shift64(audio, value)
        assert ((got - want).abs() <= 1e-12 * want.abs()).all()
    units = host_shift_units()
    print(f'fp32 interpolate on the CPU: {units:.2f} units of 2^-24')
    assert 2 < units < 16


def test_the_patch_installs_them_where_the_target_has_them():
    import types

    import promonet_amd

    def stand_in(**edits):
        return types.SimpleNamespace(
            model=types.SimpleNamespace(
                HiFiGAN=None, FARGAN=None, Generator=None),
            synthesize=types.SimpleNamespace(),
            preprocess=types.SimpleNamespace(
                spectrogram=types.SimpleNamespace(),
                loudness=types.SimpleNamespace(from_audio=None, **edits)))
    full = promonet_amd.patch(stand_in(limit=None, scale=None, shift=None))
    for name in ('from_audio', 'limit', 'scale', 'shift'):
        assert getattr(full.preprocess.loudness, name) is \
            getattr(loudness, name)
    bare = promonet_amd.patch(stand_in())
    assert set(vars(bare.preprocess.loudness)) == {'from_audio'}
