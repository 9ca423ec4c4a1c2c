"""The exact resampler tests' oracle and case table (resample_oracle.py),
checked without a GPU: `fma32` against rational arithmetic, `groups` against
the library, the table's rows for the property each is there for, the chain
against the float64 convolution - and the comparison's teeth: the integer
evaluation with ONE defect planted stands in for a wrong kernel, and exact
equality rejects each on at least one table case.

Why the exact tests exist (printed by test_chain_on_the_real_banks): the
existing bound (taps + 2) 2^-24 sum |h| |x| is about 100 times the real error
of an exact fma chain, and most of a real bank is exact zeros, so a wrong read
outside its diagonal band is multiplied by 0."""
import fractions
import math

import numpy as np
import pytest
import torch

import resample_oracle as R
from promonet_amd import _lib, load
from test_cpu_resample import PAIRS, geometry, signal


# ---------------------------------------------------------------------------
# fma32
# ---------------------------------------------------------------------------
def round_to_f32(value):
    """A Fraction rounded to the nearest fp32, ties to even, as a float"""
    if value == 0:
        return 0.
    sign, value = (-1 if value < 0 else 1), abs(value)
    exponent = value.numerator.bit_length() - value.denominator.bit_length()
    if fractions.Fraction(2) ** exponent > value:
        exponent -= 1
    assert 1 <= value / fractions.Fraction(2) ** exponent < 2
    ulp = fractions.Fraction(2) ** (max(exponent, -126) - 23)
    scaled = value / ulp
    whole = scaled.numerator // scaled.denominator
    rest = scaled - whole
    if rest > fractions.Fraction(1, 2) or (
            rest == fractions.Fraction(1, 2) and whole % 2):
        whole += 1
    return sign * float(whole * ulp)


def exact_fma(a, b, c):
    F = fractions.Fraction
    return np.array([round_to_f32(F(float(u)) * F(float(v)) + F(float(w)))
                     for u, v, w in zip(a, b, c)], dtype=np.float32)


def random_triples(count):
    """a, b with random signs and exponents; c within 2^+-30 of a b, a
    quarter of them within rounding of -a b (cancellation)"""
    rng = np.random.default_rng(1)

    def draw():
        mantissa = 1 + rng.integers(0, 2 ** 23, count) * 2. ** -23
        sign = rng.choice([-1., 1.], count)
        return sign * mantissa * 2. ** rng.integers(-10, 11, count)
    a, b = draw().astype(np.float32), draw().astype(np.float32)
    scale = np.abs(a.astype(np.float64) * b) * 2. ** rng.integers(
        -30, 31, count)
    c = (draw() * scale / 2. ** 10).astype(np.float32)
    near = np.arange(count) % 4 == 0
    bump = 1 + rng.integers(-3, 4, count) * 2. ** -23
    c[near] = (-(a.astype(np.float64) * b) * bump).astype(np.float32)[near]
    return a, b, c


def planted_ties(count):
    """c = 1 + m 2^-23, a = 2^-24 (1 + 2^-23), b = 1 +- 2^-23: a b is half an
    ulp of c, plus 2^-24 (2^-22 + 2^-46) or minus 2^-70. The latter is below
    float64's last bit next to c, so the naive sum lands on the tie and then
    rounds to even, up for an odd m, where the true sum rounds down."""
    rng = np.random.default_rng(2)
    c = (1 + rng.integers(0, 2 ** 23, count) * 2. ** -23).astype(np.float32)
    a = np.full(count, 2. ** -24 * (1 + 2. ** -23), dtype=np.float32)
    b = (1 + rng.choice([-1., 1.], count) * 2. ** -23).astype(np.float32)
    return a, b, c


def test_fma32_is_one_rounding():
    half_ulp = fractions.Fraction(2) ** -24
    assert round_to_f32(1 + half_ulp) == 1.             # a tie, to even
    assert round_to_f32(1 + 3 * half_ulp) == 1 + 2. ** -22
    assert round_to_f32(3 * fractions.Fraction(2) ** -150) == 2. ** -148
    a, b, c = random_triples(20000)
    want = exact_fma(a, b, c)
    assert np.array_equal(R.fma32(a, b, c), want)
    inexact = (a.astype(np.float64) * b + c) != want
    assert inexact.any()                    # the triples do round
    a, b, c = planted_ties(4000)
    want = exact_fma(a, b, c)
    assert np.array_equal(R.fma32(a, b, c), want)
    naive = R.fma32_naive(a, b, c) != want
    print(f'naive float64 fma wrong on {naive.sum()} of {naive.size} ties')
    assert naive.any()                      # the ties bite
    # scalars and signed zeros
    assert R.fma32(2., 3., 1.) == 7.
    assert R.fma32(0., -1., 0.) == 0. and not np.signbit(R.fma32(0., -1., 0.))


# ---------------------------------------------------------------------------
# The table
# ---------------------------------------------------------------------------
def all_geometries():
    pairs = [R.real_geometry(*pair) for pair in PAIRS + R.NEW_PAIRS]
    return R.TABLE + pairs


def test_groups_agree_with_the_library():
    library = _lib.lib()
    for orig, new, width in all_geometries():
        g = R.groups(orig, new, width)
        assert g.groups >= 1, (orig, new, width)
        assert g.strides == library.pm_resample_tile(orig, new, width)
        assert g.slots == g.groups * g.half
        assert R.segment(orig, new, width) <= R.RS_LDS_FLOATS
    for pair in PAIRS:
        assert R.real_geometry(*pair) == geometry(*pair)[:3]
        assert R.real_geometry(*pair) == load.resample_geometry(*pair)[:3]
    # a refused filter is refused here too
    assert R.groups(960, 1, 5819).groups == 0
    assert R.segment(2000, 3, 96) == R.RS_LDS_FLOATS    # the last that fits
    assert library.pm_resample_tile(2000, 3, 96) == 4
    assert R.groups(2000, 3, 97).groups == 0
    assert library.pm_resample_tile(2000, 3, 97) == _lib.PM_EINVAL


def test_every_variant_is_reached():
    every = {(V, P) for V in (4, 2, 1) for P in (1, 2)}
    old = {R.variant(*R.real_geometry(*pair)[:2]) for pair in PAIRS}
    assert old == {(2, 1), (4, 2), (1, 2)}      # three of six
    new = [R.variant(*R.real_geometry(*pair)[:2]) for pair in R.NEW_PAIRS]
    assert new == R.NEW_PAIR_VARIANTS
    assert old | set(new) == every
    assert {R.variant(orig, new) for orig, new, _ in R.TABLE} == every


def test_table_rows_have_their_property():
    seen = set()

    def row(orig, new, width, V, P, tail=None):
        assert (orig, new, width) in R.TABLE
        seen.add((orig, new, width))
        g = R.groups(orig, new, width)
        assert R.variant(orig, new) == (V, P)
        if tail is not None:
            assert g.tail == tail == (2 * width + orig) % V
        return g, 2 * width + orig

    g, taps = row(4, 1, 3, 4, 1, tail=2)
    assert g.slots > R.RS_THREADS
    g, taps = row(8, 3, 4, 4, 2, tail=0)
    assert 2 * g.half == 3 + 1      # the last slot's second phase is dead
    g, taps = row(8, 3, 5, 4, 2, tail=2)
    g, taps = row(6, 5, 4, 2, 2)
    assert 2 * g.half == 5 + 1
    g, taps = row(6, 4, 3, 2, 2)
    assert 2 * g.half == 4 and math.gcd(6, 4) > 1
    g, taps = row(2, 1, 1, 2, 1)
    assert taps == 4 and g.tail == 0
    g, taps = row(3, 1, 2, 1, 1)
    assert taps == 7 and taps % 4 == 3      # the tail loop is unrolled by 4
    g, taps = row(5, 7, 3, 1, 2)
    assert 2 * g.half == 7 + 1
    g, taps = row(1, 1, 1, 1, 1)
    assert taps == 3
    g, taps = row(640, 147, 27, 4, 2)
    assert g.groups == 3 < R.RS_SLOTS // g.half == 13
    assert g.slots < R.RS_THREADS
    g, taps = row(2000, 3, 90, 4, 2)
    assert (g.groups, g.strides) == (1, 4)
    assert R.segment(2000, 3, 90) == 8180 <= R.RS_LDS_FLOATS
    g, taps = row(4, 2500, 2, 4, 2)
    assert R.RS_SLOTS // g.half == 0 and g.groups == 1
    assert g.slots == 1250 > 4 * R.RS_THREADS
    assert seen == set(R.TABLE)
    assert len(set(R.TABLE)) == len(R.TABLE)


def test_table_lengths():
    for orig, new, width in R.TABLE:
        S = R.groups(orig, new, width).strides
        lengths = R.table_lengths(orig, new, width)
        assert lengths == sorted(set(lengths)) and lengths[0] == 1
        for length in (orig, orig + 1, S * orig - 1, S * orig, S * orig + 1,
                       (2 * S + 1) * orig + 5):
            assert length in lengths
        assert (orig - 1 in lengths) == (orig > 1)
        # three tiles, and still small
        tile_out = S * new
        last = (new * lengths[-1] + orig - 1) // orig
        assert -(-last // tile_out) == 3
        assert lengths[-1] < 20000 and R.table_n_out(
            orig, new, width, lengths[-1]) < 50000
        for n_in in lengths:
            rows = R.row_lengths(orig, new, width, n_in)
            assert rows[0] == n_in and rows[1] == 0 and 0 < rows[2] <= n_in


def test_integer_cases_are_exact():
    for orig, new, width in R.TABLE:
        taps = 2 * width + orig
        assert R.BANK_MAX * R.X_MAX * taps < 2 ** R.EXACT_BITS
        for n_in in R.table_lengths(orig, new, width):
            x, bank = R.integer_case(orig, new, width, n_in)
            assert x.shape == (R.ROWS, n_in) and bank.shape == (new, taps)
            assert np.abs(x).max() <= R.X_MAX
            assert np.abs(bank).max() <= R.BANK_MAX
            again = R.integer_case(orig, new, width, n_in)
            assert np.array_equal(x, again[0])
            assert np.array_equal(bank, again[1])
        # unlike a real bank, weight in every row and column
        if bank.size >= 1000:
            assert (bank != 0).any(0).all() and (bank != 0).any(1).all()
            assert (bank != 0).sum() > bank.size / 2
        n_out = R.table_n_out(orig, new, width, n_in)
        out = R.integer_outputs(x[0], bank, orig, new, width, n_in, n_out)
        assert np.array_equal(out, np.round(out))
        assert np.abs(out).max() < 2 ** R.EXACT_BITS
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)


def test_integer_outputs_against_the_chain():
    """The two evaluations of the oracle agree where both are exact: the fp32
    fma chain on integer data, in either order"""
    for orig, new, width in [(8, 3, 5), (3, 1, 2), (6, 5, 4), (640, 147, 27)]:
        n_in = R.table_lengths(orig, new, width)[-2]
        x, bank = R.integer_case(orig, new, width, n_in)
        n_out = R.table_n_out(orig, new, width, n_in)
        for row, length in enumerate(R.row_lengths(orig, new, width, n_in)):
            want = R.integer_outputs(
                x[row], bank, orig, new, width, length, n_out)
            for descending in (False, True):
                got = R.chain(x[row], bank, orig, new, width, length, n_out,
                              descending=descending)
                assert np.array_equal(got.astype(np.float64), want)


# ---------------------------------------------------------------------------
# Real banks
# ---------------------------------------------------------------------------
def convolution64(x, kernels, orig, new, width):
    """(value, sum of absolute products) in float64 from the fp32 bank (as
    test_gpu_resample.convolution64, one row)"""
    bank = kernels.to(torch.float64)
    length, taps = x.shape[-1], bank.shape[-1]
    n = torch.arange(-(-new * length // orig))[:, None]
    m = (n // new) * orig - width + torch.arange(taps)[None]
    inside = (m >= 0) & (m < length)
    products = x.to(torch.float64)[m.clamp(0, length - 1)] * inside
    products = products * bank[(n % new)[:, 0]]
    return products.sum(-1), products.abs().sum(-1)


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_chain_on_the_real_banks(orig_freq, new_freq):
    kernels, orig, new, width = load.resample_bank(orig_freq, new_freq)
    kernels = kernels[:, 0]
    taps = 2 * width + orig
    length = 4097
    x = signal(length)
    target = -(-new * length // orig)
    got = R.chain(x, kernels, orig, new, width, length, target + 3)
    assert got.dtype == np.float32 and not got[target:].any()
    want, scale = convolution64(x, kernels, orig, new, width)
    bound = (taps + 2) * 2. ** -24 * scale
    error = (torch.from_numpy(got[:target]).to(torch.float64) - want).abs()
    assert (error <= bound).all()
    # the order is part of the contract: the other one gives other bits
    other = R.chain(x, kernels, orig, new, width, length, target + 3,
                    descending=True)
    differing = int((other != got).sum())
    assert differing >= 1
    # the window is clamped at +-6 lobes = 12 orig / base input samples of
    # the 12 orig / base + orig a filter spans: where min(orig, new) is above
    # 12 / 0.99 most of the bank is exact zeros, and a wrong read outside its
    # band is invisible to every test on a real bank. (The two pairs below
    # that, 2 / 1 and 1 / 2, are dense.)
    nonzero = int((kernels != 0).sum())
    assert (nonzero < kernels.numel() / 2) == (min(orig, new) > 12 / .99)
    assert min(orig, new) > 12 / .99 or (orig, new) in ((2, 1), (1, 2))
    ratio = (error / bound).max().item()
    print(f'{orig_freq} -> {new_freq}: chain at {ratio:.4f} of the bound;'
          f' descending k differs in {differing} of {target}; '
          f'{kernels.numel() - nonzero} of {kernels.numel()} bank entries '
          'are zero')


# ---------------------------------------------------------------------------
# Planted defects
# ---------------------------------------------------------------------------
def table_cases():
    for orig, new, width in R.TABLE:
        for n_in in R.table_lengths(orig, new, width):
            x, bank = R.integer_case(orig, new, width, n_in)
            n_out = R.table_n_out(orig, new, width, n_in)
            lengths = R.row_lengths(orig, new, width, n_in)
            yield (orig, new, width), x, bank, lengths, n_out


@pytest.fixture(scope='module')
def clean():
    """The defect-free outputs of every table case, computed once"""
    return [
        [R.integer_outputs(x[row], bank, *triple, length, n_out)
         for row, length in enumerate(lengths)]
        for triple, x, bank, lengths, n_out in table_cases()]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_clean_outputs(clean):
    for (triple, x, bank, lengths, n_out), outputs in zip(
            table_cases(), clean):
        orig, new, width = triple
        for row, length in enumerate(lengths):
            out = outputs[row]
            out_len = -(-new * length // orig)
            assert out.shape == (n_out,) and not np.isnan(out).any()
            assert not out[out_len:].any()
            # a plain restatement of the sum, without the kernel's indexing
            for n in {0, out_len // 2, out_len - 1} - {-1}:
                q, p = divmod(n, new)
                want = sum(
                    int(bank[p, k]) * int(x[row, q * orig + k - width])
                    for k in range(2 * width + orig)
                    if 0 <= q * orig + k - width < length)
                assert out[n] == want, (triple, length, n)


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_planted_defect_is_rejected(clean, defect):
    rejecting, total = {}, 0
    for (triple, x, bank, lengths, n_out), outputs in zip(
            table_cases(), clean):
        for row, length in enumerate(lengths):
            total += 1
            wrong = R.integer_outputs(
                x[row], bank, *triple, length, n_out, defect=defect)
            if not same(wrong, outputs[row]):
                rejecting[triple] = rejecting.get(triple, 0) + 1
                at = R.first_difference(
                    wrong[None], outputs[row][None], triple[1])
                assert at is not None and at[0] == 0
    print(f'{defect}: rejected by {sum(rejecting.values())} of {total} rows, '
          f'{len(rejecting)} of {len(R.TABLE)} geometries')
    assert rejecting, defect
    # and by every variant the defect can exist in
    variants = {R.variant(*triple[:2]) for triple in rejecting}
    every = {(V, P) for V in (4, 2, 1) for P in (1, 2)}
    if defect == 'tail dropped':
        # orig is even where V = 2, and so is taps = 2 width + orig
        every = {(V, P) for V, P in every if V == 4}
    if defect in ('second phase uses p + half - 1',
                  'dead phase written over its neighbour'):
        every = {(V, P) for V, P in every if P == 2}
    assert variants == every, (defect, variants)


def test_first_difference():
    a = np.array([[1., np.nan, 3., 4.], [5., 6., 7., 8.]])
    assert R.first_difference(a, a.copy(), 3) is None
    b = a.copy()
    b[1, 2] = np.nan
    assert R.first_difference(a, b, 2)[:3] == (1, 1, 0)
