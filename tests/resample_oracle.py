"""Oracle and case table of the exact resampler tests
(test_cpu_resample_exact.py, test_gpu_resample_exact.py). numpy / torch only.

pm_resample.h promises that output n = q new + p of a row is ONE fp32
accumulator, started at 0, and the fma chain

    acc = fma(bank[p][k], x[q orig + k - width], acc),   k = 0 .. taps - 1,

in ascending k, with x = 0 outside [0, length) and zeros from
ceil(new length / orig) on. `chain` evaluates exactly that, with `fma32` an
exact fp32 fma built from float64 operations, so the device is compared with
`torch.equal` on real banks. `integer_outputs` evaluates the same sum on small
integers, where it is exact in fp32 in any order, through the kernel's own
decomposition of an output index (tile, stride group, chain, phase pair): that
is where the planted defects of the CPU test live.

`variant` and `groups` restate the dispatch of pm_audio.hip and
pm_resample_groups; the CPU test holds them to pm_resample_tile.
"""
import collections
import math

import numpy as np

# pm_resample.h
RS_THREADS = 256
RS_CHAINS = 4
RS_PHASES = 2
RS_SLOTS = 1024
RS_LDS_FLOATS = 8192

F32_MIN_NORMAL = 2. ** -126


def variant(orig, new):
    """(V, P) of the pm_resample_kernel<V, P> that pm_resample launches"""
    V = 4 if orig % 4 == 0 else 2 if orig % 2 == 0 else 1
    return V, 1 if new < RS_PHASES else RS_PHASES


Geometry = collections.namedtuple(
    'Geometry', 'groups strides half slots tail')


def groups(orig, new, width):
    """pm_resample_groups and what the launch derives from it: stride groups
    per workgroup, strides per tile, ceil(new / phases per thread), (phase,
    stride group) slots per workgroup and taps % V. groups = 0: refused."""
    taps = 2 * width + orig
    V, P = variant(orig, new)
    half = (new + P - 1) // P
    count = RS_SLOTS // half if RS_SLOTS // half > 1 else 1
    if taps > RS_LDS_FLOATS:
        return Geometry(0, 0, half, 0, taps % V)
    fit = ((RS_LDS_FLOATS - taps) // orig + 1) // RS_CHAINS
    count = min(fit, count)
    return Geometry(count, RS_CHAINS * count, half, count * half, taps % V)


def segment(orig, new, width):
    """Floats of LDS a workgroup stages"""
    return (groups(orig, new, width).strides - 1) * orig + 2 * width + orig


# ---------------------------------------------------------------------------
# One exact fp32 fma
# ---------------------------------------------------------------------------
def fma32(a, b, c):
    """round_to_fp32(a b + c) of fp32 arrays, rounded once. The product of two
    24-bit significands is exact in float64. The sum is rounded to odd there
    (TwoSum gives the residual; an inexact sum with an even last bit moves one
    ulp toward it), which keeps in its last bit what the final rounding to 24
    bits needs to know: 53 >= 24 + 2. The naive float32(a64 * b64 + c64)
    rounds twice and breaks ties the wrong way (planted in the CPU test)."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    product = a * b
    total = product + c
    virtual = total - product
    residual = (product - (total - virtual)) + (c - virtual)
    even = (np.atleast_1d(total).view(np.int64) & 1) == 0
    even = even.reshape(np.shape(total))
    toward = np.where(residual > 0, np.inf, -np.inf)
    odd = np.where((residual != 0) & even, np.nextafter(total, toward), total)
    return odd.astype(np.float32)


def fma32_naive(a, b, c):
    """What not to use: two roundings"""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64)
               for t in (a, b, c))
    return (a * b + c).astype(np.float32)


# ---------------------------------------------------------------------------
# The documented chain, on real banks
# ---------------------------------------------------------------------------
def _row(x):
    return np.asarray(x.numpy() if hasattr(x, 'numpy') else x)


def chain(x, bank, orig, new, width, length, n_out, descending=False,
          fma=fma32):
    """fp32 (n_out,): the contract of pm_resample.h for one row x (n_in,)
    that ends at `length`, bank (new, taps). `descending` runs k the other
    way (the CPU test shows that this changes bits)."""
    x = _row(x).astype(np.float32)
    bank = _row(bank).astype(np.float32)
    taps = 2 * width + orig
    assert bank.shape == (new, taps)
    length = min(max(int(length), 0), x.shape[0])
    out_len = (new * length + orig - 1) // orig
    assert n_out >= out_len
    out = np.zeros(n_out, dtype=np.float32)
    n = np.arange(out_len)
    q, p = n // new, n % new
    acc = np.zeros(out_len, dtype=np.float32)
    padded = np.concatenate([x[:length], np.zeros(1, np.float32)])
    for k in (range(taps - 1, -1, -1) if descending else range(taps)):
        index = q * orig + k - width
        inside = (index >= 0) & (index < length)
        sample = padded[np.where(inside, index, length)]
        tap = bank[p, k]
        acc = fma(tap, sample, acc)
        # nothing here may depend on how the device treats denormals
        product = np.abs(tap.astype(np.float64) * sample.astype(np.float64))
        assert not ((product != 0) & (product < F32_MIN_NORMAL)).any(), k
        assert not ((acc != 0) & (np.abs(acc) < F32_MIN_NORMAL)).any(), k
    out[:out_len] = acc
    return out


# ---------------------------------------------------------------------------
# The geometry table: (orig, new, width) passed straight through the C ABI
# (the kernel needs no sinc and no coprime rates). The CPU test asserts the
# property each row is here for.
# ---------------------------------------------------------------------------
TABLE = [
    (4, 1, 3),          # <4,1>, taps % 4 == 2, slots > 256
    (8, 3, 4),          # <4,2>, taps % 4 == 0, odd new: a dead second phase
    (8, 3, 5),          # <4,2>, taps % 4 == 2
    (6, 5, 4),          # <2,2>, odd new
    (6, 4, 3),          # <2,2>, even new, rates not coprime
    (2, 1, 1),          # <2,1>, the shortest filter
    (3, 1, 2),          # <1,1>, taps 7: the unrolled tail ends on 3
    (5, 7, 3),          # <1,2>, odd new
    (1, 1, 1),          # taps 3, degenerate
    (640, 147, 27),     # groups capped by the LDS fit at 3, slots < 256
    (2000, 3, 90),      # the cap at its minimum: 1 group, 8 180 floats
    (4, 2500, 2),       # RS_SLOTS / half == 0; 1 250 slots over 256 threads
]

# the rate pairs that reach the three variants test_cpu_resample.PAIRS never
# launches: <4,1>, <2,2>, <1,1>
NEW_PAIRS = [(88200, 22050), (14700, 22050), (66150, 22050)]
NEW_PAIR_VARIANTS = [(4, 1), (2, 2), (1, 1)]

ROWS = 3
X_PAD = 7               # x_stride = n_in + X_PAD
OUT_PAD = 5             # out_stride = n_out + OUT_PAD
BANK_MAX, X_MAX = 7, 9
EXACT_BITS = 22         # |partial sums| < 63 taps < 2^22


def table_lengths(orig, new, width):
    """Lengths around a stride's and a tile's edge, and one in the third
    tile"""
    S = groups(orig, new, width).strides
    lengths = [1, orig - 1, orig, orig + 1, S * orig - 1, S * orig,
               S * orig + 1, (2 * S + 1) * orig + 5]
    return sorted({length for length in lengths if length > 0})


def table_n_out(orig, new, width, n_in):
    """One tile and 3 samples more than ceil(new n_in / orig)"""
    S = groups(orig, new, width).strides
    return (new * n_in + orig - 1) // orig + S * new + 3


def row_lengths(orig, new, width, n_in):
    """The ragged rows of a table case: the whole row, an empty one and the
    table length before n_in (n_in itself for the shortest)"""
    lengths = table_lengths(orig, new, width)
    at = lengths.index(n_in)
    return [n_in, 0, lengths[at - 1] if at else n_in]


def integer_case(orig, new, width, n_in):
    """(x int64 (ROWS, n_in) in -9 .. 9, bank int64 (new, taps) in -7 .. 7
    without 0: every (phase, tap) pair has weight), seeded by the case"""
    rng = np.random.default_rng([orig, new, width, n_in])
    x = rng.integers(-X_MAX, X_MAX + 1, size=(ROWS, n_in))
    bank = rng.integers(1, BANK_MAX + 1, size=(new, 2 * width + orig))
    bank *= rng.choice([-1, 1], size=bank.shape)
    return x, bank


DEFECTS = [
    'last tap dropped', 'first tap dropped', 'tail dropped',
    'x read at width + 1', 'x read at width - 1',
    'second phase uses p + half - 1', 'live last phase not written',
    'dead phase written over its neighbour',
    'stride group j reads the segment of j - 1',
    'last partial stride zeroed', 'zero tail not written']


def integer_outputs(x, bank, orig, new, width, length, n_out, defect=None):
    """float64 (n_out,) of one integer row: what pm_resample leaves in
    out[0 : n_out) that was pre-filled with NaN. Plain int64 sums, indexed the
    way the kernel indexes (tile, stride group g, chain j, phase pair i), so
    that `defect` (one of DEFECTS) can go where a kernel bug would."""
    assert defect is None or defect in DEFECTS
    x, bank = np.asarray(x, dtype=np.int64), np.asarray(bank, dtype=np.int64)
    taps = 2 * width + orig
    assert bank.shape == (new, taps)
    geometry = groups(orig, new, width)
    V, P = variant(orig, new)
    half, S = geometry.half, geometry.strides
    length = min(max(int(length), 0), x.shape[0])
    out_len = (new * length + orig - 1) // orig
    assert n_out >= out_len

    n = np.arange(n_out)
    q, p = n // new, n % new
    i = p // half                           # which phase of its thread
    j = (q % S) // geometry.groups          # which chain of its thread
    computed = (q // S) * S * new < out_len     # tile not wholly past the row

    first, last = 0, taps
    if defect == 'last tap dropped':
        last = taps - 1
    if defect == 'first tap dropped':
        first = 1
    if defect == 'tail dropped' and V > 1:
        last = taps - taps % V
    shift = width + {'x read at width + 1': 1,
                     'x read at width - 1': -1}.get(defect, 0)
    staged = length
    if defect == 'last partial stride zeroed':
        staged = length - length % orig
    phase = p.copy()
    if defect == 'second phase uses p + half - 1':
        phase[i == 1] -= 1
    stride = q.copy()
    if defect == 'stride group j reads the segment of j - 1':
        stride[j >= 1] -= geometry.groups

    def values(stride, phase):
        k = np.arange(first, last)
        index = stride[:, None] * orig + k[None] - shift
        inside = (index >= 0) & (index < staged)
        padded = np.concatenate([x, np.zeros(1, np.int64)])
        samples = padded[np.where(inside, index, x.shape[0])]
        return (bank[phase][:, first:last] * samples).sum(1)

    out = np.full(n_out, np.nan)
    body = n < out_len
    out[body] = values(stride[body], phase[body])
    out[~body] = 0.
    if defect == 'zero tail not written':
        out[~body] = np.nan
    if defect == 'live last phase not written':
        # (a tile wholly past the row zero-fills without its phases)
        out[(p == new - 1) & computed] = np.nan
    if (defect == 'dead phase written over its neighbour' and
            P * half > new):
        # the slot p = half - 1 of stride q repeats phase half - 1 in its
        # second lane and would store it at q new + 2 half - 1 = (q + 1) new
        assert P == 2 and 2 * half == new + 1
        target = (p == 0) & (q >= 1) & body
        out[target] = values(q[target] - 1, np.full(target.sum(), half - 1))
    return out


def first_difference(got, want, new):
    """(row, q, p, got, want) of the first entry where two (rows, n) arrays
    differ (NaN equals NaN), or None"""
    got, want = np.asarray(got), np.asarray(want)
    differ = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not differ.any():
        return None
    row, n = (int(v) for v in np.argwhere(differ)[0])
    return row, n // new, n % new, got[row, n].item(), want[row, n].item()


def real_geometry(orig_freq, new_freq):
    """(orig, new, width) of a rate pair, as load.resample_geometry"""
    gcd = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // gcd, new_freq // gcd
    return orig, new, math.ceil(6 * orig / (min(orig, new) * .99))
