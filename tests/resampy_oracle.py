"""Oracle of the interpolated-sinc resampler tests (test_cpu_augment.py,
test_gpu_augment.py). numpy only; shares nothing with promonet_amd.resampy.

Three evaluations of resampy's resample_f, as published and as recalled:

  `literal64`   the loop of the package with FLOAT positions: time = t (orig /
                new), n = int(time), frac = scale (time - n), ... in float64
  `contract64`  the contract of include/promonet_hip.h (positions in
                integers) in float64, tables and eta unrounded
  `chain32`     the contract in fp32: tables and eta rounded, every weight one
                fma, every output ONE accumulator and one fma per tap, left
                wing then right wing, ascending; `fma32` is an exact fp32 fma

and `integer_outputs`, the contract on small integers, where every sum is exact
in fp32 in any order; the planted defects of the CPU test live there.
"""
import math

import numpy as np

from resample_oracle import F32_MIN_NORMAL, fma32

P = 512
ZEROS = 64
N = ZEROS * P
# resampy's published 'kaiser_best' parameters, as recalled
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492

# the kernel's tile (pm_resample_interp.h; the CPU test holds it to
# pm_resample_interp_tile)
TILE = 1024
LDS_FLOATS = 6144

# rate pairs of the device tests and what each reaches
PAIRS = [
    (48000, 22050),     # down, step 235
    (54441, 44100),     # down, coprime-ish
    (22050, 44100),     # up, rem in {0, new / 2}
    (22051, 22050),     # what the polyphase path refuses
    (24000, 48000),     # pitch extreme, ratio 0.5
    (96000, 48000),     # pitch extreme, ratio 2
]
# D = max(orig, new) a power of two: eta is dyadic and integer tables give
# exact sums. rem P mod D is a multiple of P for D = 2^k >= P, so eta takes
# D / P values: 16 of them at D = 8192, with every rem occurring (the other
# rate is odd). At D <= P (the last three) eta is always 0: they are kept for
# their ratios, and do not see eta at all.
INTEGER_PAIRS = [(6145, 8192), (8192, 6145), (8192, 2049), (2049, 8192),
                 (48, 64), (64, 48), (32, 128)]


def tables64(orig=1, new=1):
    """(win, delta) in float64, N + 1 entries each. The Kaiser window is
    written out (I0 of the half window), not taken from numpy's kaiser."""
    j = np.arange(N + 1, dtype=np.float64)
    taper = np.i0(BETA * np.sqrt(1 - (j / N) ** 2)) / np.i0(BETA)
    win = ROLLOFF * np.sinc(ROLLOFF * j / P) * taper
    if new < orig:
        win = win * (new / orig)
    delta = np.append(win[1:] - win[:-1], 0.)
    return win, delta


def tables32(orig=1, new=1):
    return tuple(table.astype(np.float32) for table in tables64(orig, new))


def step_of(orig, new):
    return min(orig, new) * P // orig


def wing_of(orig, new):
    """The longest wing: taps either side of an output"""
    return (N + 1) // step_of(orig, new)


def positions(t, orig, new):
    """The integers of the contract for outputs t (int64 array): n, and per
    wing (off, numerator of eta over D)"""
    t = np.asarray(t, dtype=np.int64)
    n, rem = t * orig // new, t * orig % new
    D = max(orig, new)
    return n, rem, D, (rem * P // D, rem * P % D), (
        (new - rem) * P // D, (new - rem) * P % D)


def lengths_of(orig, new):
    """1, 2, the longest wing +- 1, the inputs of one tile of outputs +- 1 and
    a length whose last output is in the third tile"""
    wing = wing_of(orig, new)
    tile_in = -(-TILE * orig // new)
    lengths = [1, 2, wing - 1, wing + 1, tile_in - 1, tile_in + 1,
               5 * tile_in // 2 + 3]
    return sorted({length for length in lengths if length > 0})


def signal(length, seed=0):
    """fp32 uniform in [-1, 1] with +-1 at the first and the last sample"""
    rng = np.random.default_rng([length, seed])
    x = rng.uniform(-1, 1, size=length)
    x[0], x[-1] = 1., -1.
    return x.astype(np.float32)


# ---------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------
def literal64(x, orig, new):
    """resampy's loop with float positions. Returns (y float64, offsets): the
    (left, right) table offsets of every output, for the comparison with the
    integer positions."""
    x = np.asarray(x, dtype=np.float64)
    win, delta = tables64(orig, new)
    sample_ratio = new / orig
    scale = min(1., sample_ratio)
    time_increment = 1. / sample_ratio
    index_step = int(scale * P)
    n_orig = x.shape[0]
    n_out = int(n_orig * sample_ratio)
    y = np.zeros(n_out)
    offsets = np.zeros((n_out, 2), dtype=np.int64)
    for t in range(n_out):
        time_register = t * time_increment
        n = int(time_register)
        frac = scale * (time_register - n)
        index_frac = frac * P
        offset = int(index_frac)
        eta = index_frac - offset
        offsets[t, 0] = offset
        i = np.arange(min(n + 1, (N + 1 - offset) // index_step))
        at = offset + i * index_step
        y[t] += ((win[at] + eta * delta[at]) * x[n - i]).sum()
        frac = scale - frac
        index_frac = frac * P
        offset = int(index_frac)
        eta = index_frac - offset
        offsets[t, 1] = offset
        k = np.arange(min(n_orig - n - 1, (N + 1 - offset) // index_step))
        at = offset + k * index_step
        y[t] += ((win[at] + eta * delta[at]) * x[n + k + 1]).sum()
    return y, offsets


def _wings(x, orig, new, n_win=N + 1):
    """Per wing: (off, eta numerator, count, tap index matrix, sample index
    matrix, live mask) for every output of a row x"""
    length = x.shape[0]
    t = np.arange(length * new // orig, dtype=np.int64)
    n, rem, D, left, right = positions(t, orig, new)
    step = step_of(orig, new)
    for (off, m), count, first, direction in (
            (left, n + 1, n, -1), (right, length - n - 1, n + 1, 1)):
        count = np.minimum(count, (n_win - off) // step)
        i = np.arange(int(count.max(initial=0)), dtype=np.int64)[None]
        live = i < count[:, None]
        at = np.where(live, off[:, None] + i * step, 0)
        index = np.where(live, first[:, None] + direction * i, 0)
        yield off, m, D, count, at, index, live


def contract64(x, orig, new):
    """The contract in float64 with unrounded tables. Returns (y, sum of
    |w_k| |x_k|, sum of |eta_k delta_k| |x_k|, taps) per output, and the
    (left, right) offsets."""
    x = np.asarray(x, dtype=np.float64)
    win, delta = tables64(orig, new)
    outputs = x.shape[0] * new // orig
    y, scale, slope = (np.zeros(outputs) for _ in range(3))
    taps = np.zeros(outputs, dtype=np.int64)
    offsets = []
    for off, m, D, count, at, index, live in _wings(x, orig, new):
        eta = (m / D)[:, None]
        w = (win[at] + eta * delta[at]) * live
        y += (w * x[index]).sum(1)
        scale += np.abs(w * x[index]).sum(1)
        slope += np.abs(eta * delta[at] * live * x[index]).sum(1)
        taps += count
        offsets.append(off)
    return y, scale, slope, taps, np.stack(offsets, 1)


# ---------------------------------------------------------------------------
# fp32
# ---------------------------------------------------------------------------
def chain32(x, orig, new, win, delta, length=None, n_out=None,
            descending=False):
    """fp32 (n_out,): the contract for one row x that ends at `length`, with
    fp32 tables (win, delta). `descending` walks each wing from its last tap
    to its first (the CPU test shows that this changes bits)."""
    x = np.asarray(x, dtype=np.float32)
    length = x.shape[0] if length is None else min(max(int(length), 0),
                                                    x.shape[0])
    x = x[:length]
    outputs = length * new // orig
    n_out = outputs if n_out is None else n_out
    assert n_out >= outputs
    acc = np.zeros(outputs, dtype=np.float32)
    for off, m, D, count, at, index, live in _wings(x, orig, new, win.shape[0]):
        eta = m.astype(np.float32) / np.float32(D)
        columns = range(at.shape[1])
        for i in (reversed(columns) if descending else columns):
            mask = live[:, i]
            weight = fma32(eta, delta[at[:, i]], win[at[:, i]])
            sample = x[index[:, i]]
            value = fma32(weight, sample, acc)
            # nothing here may depend on how the device treats denormals
            product = np.abs(weight.astype(np.float64) * sample)[mask]
            assert not ((product != 0) & (product < F32_MIN_NORMAL)).any(), i
            acc = np.where(mask, value, acc)
            assert not ((acc != 0) & (np.abs(acc) < F32_MIN_NORMAL)).any(), i
    out = np.zeros(n_out, dtype=np.float32)
    out[:outputs] = acc
    return out


# ---------------------------------------------------------------------------
# Small integers: exact in any order
# ---------------------------------------------------------------------------
TABLE_MAX, X_MAX = 7, 9
DEFECTS = [
    'left first tap dropped', 'right first tap dropped',
    'left last tap dropped', 'right last tap dropped',
    'left wing reads x[n - i - 1]', 'right wing starts at x[n]',
    'eta and eta\' swapped', 'off\' formed from rem',
    'step taken as P when downsampling', 'last partial output written',
    'zero tail not written', 'a tile reads its neighbour\'s segment']


def integer_case(orig, new, rows, n_in):
    """(x (rows, n_in) in -9 .. 9, win, delta in +-1 .. 7 without zero, all
    int64), seeded by the case"""
    rng = np.random.default_rng([orig, new, rows, n_in])
    x = rng.integers(-X_MAX, X_MAX + 1, size=(rows, n_in))
    tables = rng.integers(1, TABLE_MAX + 1, size=(2, N + 1))
    tables *= rng.choice([-1, 1], size=tables.shape)
    return x, tables[0], tables[1]


def integer_outputs(x, win, delta, orig, new, length, n_out, defect=None):
    """float64 (n_out,) of one integer row: what pm_resample_interp leaves in
    out[0 : n_out) that was pre-filled with NaN. D must be a power of two:
    the sum of (win D + m delta) x is an int64 and its quotient by D exact.
    `defect` (one of DEFECTS) goes where a kernel bug would."""
    assert defect is None or defect in DEFECTS
    D = max(orig, new)
    assert D & (D - 1) == 0
    x = np.asarray(x, dtype=np.int64)
    length = min(max(int(length), 0), x.shape[0])
    padded = np.concatenate([x[:length], np.zeros(1, np.int64)])
    outputs = length * new // orig
    if defect == 'last partial output written':
        outputs = -(-length * new // orig)
    outputs = min(outputs, n_out)
    t = np.arange(outputs, dtype=np.int64)
    n, rem, D, (off, m), (off2, m2) = positions(t, orig, new)
    step = step_of(orig, new)
    if defect == 'step taken as P when downsampling':
        step = P
    if defect == 'eta and eta\' swapped':
        m, m2 = m2, m
    if defect == 'off\' formed from rem':
        off2 = off
    shift = np.zeros_like(n)
    if defect == 'a tile reads its neighbour\'s segment':
        # tile k >= 1 stages the samples around tile k - 1's first output
        first = (t // TILE) * TILE
        shift = np.where(first > 0,
                         first * orig // new - (first - TILE) * orig // new, 0)
    total, largest = (np.zeros(outputs, dtype=np.int64) for _ in range(2))
    for side, off_, m_, count, first, direction in (
            ('left', off, m, n + 1, n, -1),
            ('right', off2, m2, length - n - 1, n + 1, 1)):
        count = np.maximum(np.minimum(count, (N + 1 - off_) // step), 0)
        if defect == 'left wing reads x[n - i - 1]' and side == 'left':
            first = first - 1
        if defect == 'right wing starts at x[n]' and side == 'right':
            first = first - 1
        for i in range(int(count.max(initial=0))):
            live = i < count
            if defect == f'{side} first tap dropped':
                live &= i > 0
            if defect == f'{side} last tap dropped':
                live &= i < count - 1
            at = np.where(live, off_ + i * step, 0)
            index = first + direction * i - shift
            inside = live & (index >= 0) & (index < length)
            sample = padded[np.where(inside, index, length)]
            term = np.where(live, (win[at] * D + m_ * delta[at]) * sample, 0)
            total += term
            largest += np.abs(term)
    # every numerator is a multiple of gcd(P, D): every partial sum, in any
    # order, is an integer below 2^24 times gcd(P, D) / D
    assert largest.max(initial=0) // math.gcd(P, D) < 2 ** 24
    out = np.full(n_out, np.nan)
    out[:outputs] = total / D
    if defect != 'zero tail not written':
        out[outputs:] = 0.
    return out


def gcd_delay(orig, new, s):
    """(zeros to prepend, samples the output is delayed by)"""
    g = math.gcd(orig, new)
    return s * orig // g, s * new // g
