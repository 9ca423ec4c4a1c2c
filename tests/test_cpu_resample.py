"""The resampler on the host: `load.resample` against a direct float64
evaluation of the windowed-sinc formula and against a frozen copy of itself,
the argument checks of pm_resample, and the cap on the device bank. No GPU.

Error bound used here and in test_gpu_resample.py (derived, not measured): an
output of K = taps products is within (K + 2) 2^-24 sum_k |h_k| |x_k| of its
float64 value: one rounding of each tap to fp32 plus K fmas in any order.
"""
import ctypes
import math

import pytest
import torch

from promonet_amd import _lib, load

PAIRS = [(44100, 22050), (48000, 22050), (16000, 22050), (11025, 22050),
         (24000, 22050), (32000, 22050), (22050, 16000), (96000, 22050)]


def geometry(orig_freq, new_freq):
    gcd = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // gcd, new_freq // gcd
    base = min(orig, new) * .99
    return orig, new, math.ceil(6 * orig / base), base


def fixed_lengths(orig_freq, new_freq):
    """The lengths of the issue that need nothing but the rate pair"""
    orig = geometry(orig_freq, new_freq)[0]
    lengths = [1, 2, 7, orig - 1, orig, orig + 1, 5 * orig - 1, 4097]
    return sorted({length for length in lengths if length > 0})


def lengths_of(orig_freq, new_freq):
    """`fixed_lengths` and one that ends one stride past the edge of the
    kernel's first tile (asked of the library: the device tests use it)"""
    orig = geometry(orig_freq, new_freq)[0]
    strides, _ = load.resample_tile(orig_freq, new_freq)
    return sorted(set(fixed_lengths(orig_freq, new_freq)) |
                  {(strides + 1) * orig})


def signal(length, seed=0):
    """Uniform in [-1, 1] with +-1 at the first and the last sample"""
    gen = torch.Generator().manual_seed(1000 * seed + length)
    x = torch.rand(length, generator=gen, dtype=torch.float64) * 2 - 1
    x[0], x[-1] = 1., -1.
    return x.to(torch.float32)


def formula(x, orig_freq, new_freq):
    """out[n] = sum_m x[m] g((m new - n orig) / (orig new)) in float64, with
    g(t) = sinc(pi c) cos^2(pi c / 12) base / orig, c = clamp(base t, +-6);
    (value, sum of absolute products, taps)"""
    orig, new, width, base = geometry(orig_freq, new_freq)
    length, taps = x.shape[-1], 2 * width + orig
    target = -(-new * length // orig)
    n = torch.arange(target, dtype=torch.int64)[:, None]
    # g vanishes where |base t| >= 6 (the window's zero), which is outside
    # m = q orig - width + k, k in [0, taps), for n = q new + p: only those
    # m are visited
    m = (n // new) * orig - width + torch.arange(taps, dtype=torch.int64)[None]
    numerator = m * new - n * orig                       # integers
    t = numerator.to(torch.float64) / (orig * new)
    c = (t * base).clamp(-6, 6)
    window = torch.cos(c * math.pi / 12) ** 2
    c = c * math.pi
    g = torch.where(c == 0, torch.ones_like(c), c.sin() / c)
    g = g * window * (base / orig)
    inside = (m >= 0) & (m < length)
    products = g * x.to(torch.float64)[m.clamp(0, length - 1)] * inside
    return products.sum(1), products.abs().sum(1), taps


def frozen_resample(waveform, orig_freq, new_freq, lowpass_filter_width=6,
                    rolloff=.99):
    """`load.resample` as it stood before the bank was factored out; returns
    (output, kernels)"""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    gcd = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // gcd, new_freq // gcd
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    index = torch.arange(
        -width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(
        0, -new, -1, dtype=torch.float64)[:, None, None] / new + index
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t)
    kernels = (kernels * window * (base / orig)).to(torch.float32)
    shape = waveform.shape
    flat = waveform.reshape(-1, shape[-1]).to(torch.float32)
    length = flat.shape[-1]
    padded = torch.nn.functional.pad(flat, (width, width + orig))
    out = torch.nn.functional.conv1d(padded[:, None], kernels, stride=orig)
    out = out.transpose(1, 2).reshape(flat.shape[0], -1)
    target = int(math.ceil(new * length / orig))
    return out[..., :target].reshape(shape[:-1] + (target,)), kernels


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_host_path_against_the_formula(orig_freq, new_freq):
    orig, new, width, _ = geometry(orig_freq, new_freq)
    worst = 0.
    for length in fixed_lengths(orig_freq, new_freq):
        x = signal(length)
        got = load.resample(x[None], orig_freq, new_freq)
        want, scale, taps = formula(x, orig_freq, new_freq)
        assert got.shape == (1, -(-new * length // orig))
        assert got.dtype == torch.float32
        bound = (taps + 2) * 2. ** -24 * scale
        error = (got[0].to(torch.float64) - want).abs()
        worst = max(worst, (error / bound).max().item())
        assert (error <= bound).all(), (length, (error / bound).max().item())
    print(f'{orig_freq} -> {new_freq}: worst error / bound {worst:.3f}')


@pytest.mark.parametrize(
    'orig_freq,new_freq', [(44100, 22050), (48000, 22050), (16000, 22050)])
def test_host_path_is_frozen(orig_freq, new_freq):
    orig = geometry(orig_freq, new_freq)[0]
    x = torch.stack([signal(5 * orig + 3, seed) for seed in range(3)])
    want, kernels = frozen_resample(x, orig_freq, new_freq)
    got = load.resample(x, orig_freq, new_freq)
    assert got.shape == want.shape and torch.equal(got, want)
    # a (2, 3, n) float64 input takes the same cast and the same reshape
    deep = torch.stack([x, -x]).to(torch.float64)
    assert torch.equal(
        load.resample(deep, orig_freq, new_freq),
        frozen_resample(deep, orig_freq, new_freq)[0])
    bank = load.resample_bank(orig_freq, new_freq)
    assert torch.equal(bank[0], kernels) and bank[0].dtype == torch.float32
    assert bank[1:] == geometry(orig_freq, new_freq)[:3]
    assert kernels.shape == (bank[2], 1, 2 * bank[3] + bank[1])
    assert load.resample(x, 22050, 22050) is x


def test_geometry_table():
    """The table of the issue: orig / new, width, taps"""
    for rate, want in {44100: (2, 1, 13, 28), 48000: (320, 147, 14, 348),
                       16000: (320, 441, 7, 334), 32000: (640, 441, 9, 658),
                       96000: (640, 147, 27, 694),
                       11025: (1, 2, 7, 15)}.items():
        orig, new, width, _ = load.resample_geometry(rate, 22050)
        assert (orig, new, width, 2 * width + orig) == want, rate


def call(library, **overrides):
    """pm_resample with valid sizes and fake, never dereferenced, pointers"""
    a = dict(x=0x1000, lengths=None, bank=0x2000, out=0x3000, rows=2,
             n_in=1000, x_stride=1000, orig=320, new=147, width=14,
             n_out=460, out_stride=460)
    a.update(overrides)
    return library.pm_resample(
        a['x'], a['lengths'], a['bank'], a['out'], a['rows'], a['n_in'],
        a['x_stride'], a['orig'], a['new'], a['width'], a['n_out'],
        a['out_stride'], None)


def test_signature_and_argument_checks():
    assert 'pm_resample' in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES['pm_resample']
    assert restype is ctypes.c_int and len(argtypes) == 13
    library = _lib.lib()
    assert math.ceil(147 * 1000 / 320) == 460
    for overrides, message in [
            (dict(rows=-1), 'negative'), (dict(n_in=-1), 'negative'),
            (dict(n_out=-1), 'negative'),
            (dict(orig=0), 'at least 1'), (dict(new=0), 'at least 1'),
            (dict(width=0), 'at least 1'),
            (dict(x=None), 'null'), (dict(bank=None), 'null'),
            (dict(out=None), 'null'),
            (dict(n_out=459, out_stride=459), 'n_out'),
            (dict(x_stride=999), 'stride'), (dict(out_stride=459), 'stride')]:
        code = call(library, **overrides)
        assert code == _lib.PM_EINVAL, overrides
        assert message in library.pm_last_error().decode(), overrides
        with pytest.raises(_lib.LibraryError):
            _lib.check(code)
    # nothing to do is not an error, and launches nothing
    assert call(library, rows=0) == 0
    assert call(library, n_in=0, x_stride=0, n_out=0, out_stride=0) == 0
    # the tile geometry comes from the library, and needs no GPU either
    assert library.pm_resample_tile(0, 1, 1) == _lib.PM_EINVAL
    # a filter too long for the kernel's LDS segment (48 kHz -> 50 Hz: 12 598
    # taps) is refused by both entries, not run some slower way
    long = load.resample_geometry(48000, 50)[:3]
    assert long == (960, 1, 5819)
    assert library.pm_resample_tile(*long) == _lib.PM_EINVAL
    assert 'LDS' in library.pm_last_error().decode()
    assert call(library, orig=960, new=1, width=5819) == _lib.PM_EINVAL
    for orig_freq, new_freq in PAIRS:
        orig, new, width, _ = geometry(orig_freq, new_freq)
        strides, outputs = load.resample_tile(orig_freq, new_freq)
        assert strides >= 1 and outputs == strides * new
        assert strides == library.pm_resample_tile(orig, new, width)


def test_bank_cap(monkeypatch):
    """22 051 -> 22 050 shares no divisor: 22 050 filters of 289 393 taps.
    The size rule speaks before anything is built."""
    orig, new, width, _ = load.resample_geometry(22051, 22050)
    assert (orig, new) == (22051, 22050)
    assert new * (2 * width + orig) > load.RESAMPLE_BANK_MAX_FLOATS
    assert load.RESAMPLE_BANK_MAX_FLOATS == 4 * 1024 * 1024

    def never(*args, **kwargs):
        raise AssertionError('the bank was being built')
    monkeypatch.setattr(torch, 'arange', never)
    with pytest.raises(ValueError, match='22051 Hz -> 22050 Hz'):
        load.resample_bank(
            22051, 22050, max_floats=load.RESAMPLE_BANK_MAX_FLOATS)
    monkeypatch.undo()
    # every standard pair is far below the cap, and builds with it
    for orig_freq, new_freq in PAIRS:
        kernels = load.resample_bank(
            orig_freq, new_freq, max_floats=load.RESAMPLE_BANK_MAX_FLOATS)[0]
        assert kernels.numel() < 300_000
