"""pm_resample bit for bit, on every kernel variant it can launch.
`torch.equal` only: there is no tolerance in this file.

Integers through the C ABI: a bank in -7 .. 7 and samples in -9 .. 9 make
every partial sum an integer below 2^22, exact in fp32 in any order, so the
expected output is a plain integer sum - and every (phase, tap) pair carries
weight, where a real bank is mostly exact zeros. The geometry table of
resample_oracle.py reaches all six pm_resample_kernel<V, P>, both tail loops,
the dead second phase of an odd `new`, both ends of the LDS cap and more slots
than threads; test_cpu_resample_exact.py plants the indexing defects that
these cases reject.

Real banks through load.resample: the header's contract - one fp32
accumulator, an fma chain over ascending k - evaluated by `chain` with an
exact fp32 fma, on the eight rate pairs of test_cpu_resample.py and the three
that reach the variants those never launch."""
import numpy as np
import pytest
import torch

import resample_oracle as R
from promonet_amd import _lib, load
from test_cpu_resample import PAIRS, lengths_of, signal

pytestmark = pytest.mark.gpu

NAN = float('nan')


def run(device, x, bank, lengths, orig, new, width, n_in, n_out):
    """pm_resample on rows of x_stride = n_in + X_PAD with NaN past each
    row's length, into NaN-filled rows of out_stride = n_out + OUT_PAD;
    returns the whole (rows, out_stride) buffer on the host"""
    rows = x.shape[0]
    staged = torch.full((rows, n_in + R.X_PAD), NAN)
    for row in range(rows):
        length = n_in if lengths is None else lengths[row]
        staged[row, :length] = torch.from_numpy(x[row, :length]).float()
    staged = staged.to(device)
    taps_major = torch.from_numpy(bank).float().T.contiguous().to(device)
    assert taps_major.shape == (2 * width + orig, new)
    device_lengths = None
    if lengths is not None:
        device_lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    out = torch.full((rows, n_out + R.OUT_PAD), NAN, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_resample(
            _lib.ptr(staged), _lib.ptr(device_lengths, torch.int32),
            _lib.ptr(taps_major), _lib.ptr(out), rows, n_in,
            n_in + R.X_PAD, orig, new, width, n_out, n_out + R.OUT_PAD,
            _lib.stream()))
    return out.cpu()


@pytest.mark.parametrize('orig,new,width', R.TABLE)
def test_integer_cases(device, orig, new, width):
    for n_in in R.table_lengths(orig, new, width):
        x, bank = R.integer_case(orig, new, width, n_in)
        n_out = R.table_n_out(orig, new, width, n_in)
        ragged = R.row_lengths(orig, new, width, n_in)
        for lengths in (None, ragged):
            want = np.stack([
                R.integer_outputs(
                    x[row], bank, orig, new, width,
                    n_in if lengths is None else lengths[row], n_out)
                for row in range(R.ROWS)])
            want = torch.from_numpy(want).float()
            got = run(device, x, bank, lengths, orig, new, width, n_in, n_out)
            # [0, n_out) is the oracle's, zero tail included ...
            assert torch.equal(got[:, :n_out], want), (
                n_in, lengths, '(row, q, p, got, want)',
                R.first_difference(got[:, :n_out].numpy(), want.numpy(), new))
            # ... and nothing past n_out was touched
            assert got[:, n_out:].isnan().all(), (n_in, lengths)


def real_case(device, orig_freq, new_freq):
    kernels, orig, new, width = load.resample_bank(orig_freq, new_freq)
    kernels = kernels[:, 0]
    assert (orig, new, width) == R.real_geometry(orig_freq, new_freq)
    lengths = lengths_of(orig_freq, new_freq)
    longest = max(lengths)
    target = -(-new * longest // orig)
    want = {length: torch.from_numpy(R.chain(
        signal(length), kernels, orig, new, width, length, target))
        for length in lengths}
    # batch 1
    for length in lengths:
        got = load.resample(signal(length)[None].to(device),
                            orig_freq, new_freq)
        valid = -(-new * length // orig)
        assert got.shape == (1, valid)
        assert torch.equal(got[0].cpu(), want[length][:valid]), (
            length, '(row, q, p, got, want)', R.first_difference(
                got.cpu().numpy(), want[length][None, :valid].numpy(), new))
    # batch 3, ragged: every length once, NaN past each row's end
    for start in range(0, len(lengths), 3):
        three = (lengths[start:start + 3] + lengths[:2])[:3]
        x = torch.full((3, longest), NAN)
        for row, length in enumerate(three):
            x[row, :length] = signal(length)
        got, got_lengths = load.resample(
            x.to(device), orig_freq, new_freq, lengths=three)
        assert got.shape == (3, target)
        assert got_lengths == [-(-new * length // orig) for length in three]
        expected = torch.stack([want[length] for length in three])
        assert torch.equal(got.cpu(), expected), (
            three, '(row, q, p, got, want)', R.first_difference(
                got.cpu().numpy(), expected.numpy(), new))


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_real_banks(device, orig_freq, new_freq):
    real_case(device, orig_freq, new_freq)


@pytest.mark.parametrize(
    'orig_freq,new_freq,V,P',
    [pair + kind for pair, kind in zip(R.NEW_PAIRS, R.NEW_PAIR_VARIANTS)])
def test_real_banks_of_the_other_variants(device, orig_freq, new_freq, V, P):
    orig, new, _ = R.real_geometry(orig_freq, new_freq)
    assert R.variant(orig, new) == (V, P)
    assert (V, P) not in {
        R.variant(*R.real_geometry(*pair)[:2]) for pair in PAIRS}
    real_case(device, orig_freq, new_freq)
