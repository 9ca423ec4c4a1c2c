"""resampy.resample('kaiser_best') on the device: band-limited sinc
interpolation at ANY ratio (promonet/data/augment/{pitch,loudness}.py call it
with int(ratio * sample_rate) -> sample_rate, ratio in [0.5, 2]).

`load.resample` (torchaudio's polyphase resampler) needs one filter per output
phase and refuses rate pairs with a small common divisor. This module reads one
long windowed-sinc table with linear interpolation at a per-output phase
(pm_resample_interp; the contract, positions in integers and one fp32 fma
chain per output, is stated in include/promonet_hip.h).

resampy is not a dependency: the algorithm and the 'kaiser_best' parameters
are written down from the published package as recalled, so parity with the
package's own output is unpinned (DESIGN.md sections 2 and 17). resampy ships
the filter as a precomputed table; here it is built from the formula.
"""
import functools

import numpy as np
import torch

import promonet_amd
from promonet_amd import _lib

# include/promonet_hip.h
PRECISION = 9
STEPS = 2 ** PRECISION              # table steps per zero crossing
NUM_ZEROS = 64
TABLE = NUM_ZEROS * STEPS + 1

# resampy's published 'kaiser_best' parameters, AS RECALLED (unpinned)
KAISER_BEST_ROLLOFF = 0.9475937167399596
KAISER_BEST_BETA = 14.769656459379492


###############################################################################
# The filter
###############################################################################


@functools.lru_cache(maxsize=None)
def _window():
    """win[0 .. N] in float64, unscaled: the right half of the Kaiser-windowed
    sinc"""
    n = TABLE - 1
    sinc = KAISER_BEST_ROLLOFF * np.sinc(
        KAISER_BEST_ROLLOFF * np.arange(n + 1, dtype=np.float64) / STEPS)
    return sinc * np.kaiser(2 * n + 1, KAISER_BEST_BETA)[n:]


def scaling(sr_orig, sr_new):
    """What the table is multiplied by: new / orig when downsampling"""
    sr_orig, sr_new = int(sr_orig), int(sr_new)
    return sr_new / sr_orig if sr_new < sr_orig else 1.


def _scaled(scale):
    """(win, delta) fp32 for a table scaling: scaled and differenced in
    float64, rounded to fp32 last"""
    win = _window() * float(scale)
    delta = np.zeros_like(win)
    delta[:-1] = win[1:] - win[:-1]
    return win.astype(np.float32), delta.astype(np.float32)


def tables(sr_orig=1, sr_new=1):
    """(win, delta): fp32 numpy arrays of TABLE entries for this rate pair"""
    return _scaled(scaling(sr_orig, sr_new))


_device_tables = {}


def device_tables(scale, device):
    """(win, delta) on `device` for a table scaling, uploaded once"""
    key = (float(scale), str(device))
    if key not in _device_tables:
        _device_tables[key] = tuple(
            torch.from_numpy(table).to(device) for table in _scaled(scale))
    return _device_tables[key]


def tile(sr_orig, sr_new):
    """Outputs one workgroup of the kernel takes for this rate pair, asked of
    the library (needs no GPU). Raises _lib.LibraryError for rates the kernel
    refuses: a ratio whose input segment does not fit its LDS."""
    outputs = _lib.lib().pm_resample_interp_tile(int(sr_orig), int(sr_new))
    if outputs < 0:
        _lib.check(outputs)
    return outputs


###############################################################################
# The call
###############################################################################


def resample(x, sr_orig, sr_new, filter='kaiser_best', lengths=None,
             gpu=None):
    """resampy.resample(x, sr_orig, sr_new) along the last axis.

    x: a tensor (..., samples) of any floating type and strides (cast to fp32);
    returns fp32 (..., samples * sr_new // sr_orig).

    sr_orig, sr_new: ints, or one int per flattened row (a list or a CPU
    tensor; they are uploaded, never read back) for a batch in which every row
    has its own ratio. `lengths` (a list or a tensor, one per flattened row)
    makes the batch ragged. With per-row rates or lengths the result is (out,
    out_lengths): row r holds lengths[r] * new[r] // orig[r] outputs and exact
    zeros after them, out_lengths a list.

    A device tensor, or any tensor with `gpu`, runs pm_resample_interp on the
    current stream; rows that share a table scaling (every upsampling row, or
    one downsampling ratio) share a launch. A CPU tensor with gpu=None is
    evaluated on the host, sample for sample the same fma chains: slow, for
    tests and hosts without a GPU."""
    if filter != 'kaiser_best':
        raise ValueError(
            f"filter {filter!r}: only 'kaiser_best' is implemented")
    x = torch.as_tensor(x)
    if gpu is not None:
        x = x.to(torch.device(f'cuda:{gpu}'))
    shape = x.shape
    samples = shape[-1]
    rows = int(np.prod(shape[:-1], dtype=np.int64))
    ragged = lengths is not None or not (
        _is_int(sr_orig) and _is_int(sr_new))
    orig = _per_row(sr_orig, rows, 'sr_orig')
    new = _per_row(sr_new, rows, 'sr_new')
    for pair in sorted(set(zip(orig, new))):
        if pair[0] < 1 or pair[1] < 1:
            raise ValueError(f'sample rates must be positive, got {pair}')
        tile(*pair)
    if lengths is None:
        row_lengths = [samples] * rows
    else:
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.reshape(-1).tolist()
        row_lengths = [min(max(int(item), 0), samples) for item in lengths]
        if len(row_lengths) != rows:
            raise ValueError(
                f'{len(row_lengths)} lengths for {rows} rows of audio')
    out_lengths = [
        length * n // o for length, o, n in zip(row_lengths, orig, new)]
    n_out = max([samples * n // o for o, n in zip(orig, new)], default=0)
    flat = x.reshape(rows, samples).to(torch.float32)
    if flat.is_cuda:
        out = _device(flat, row_lengths, orig, new, n_out)
    else:
        out = torch.zeros(rows, n_out, dtype=torch.float32)
        for row in range(rows):
            win, delta = tables(orig[row], new[row])
            out[row, :out_lengths[row]] = torch.from_numpy(host_row(
                flat[row, :row_lengths[row]].numpy(), orig[row], new[row],
                win, delta))
    out = out.reshape(shape[:-1] + (n_out,))
    return (out, out_lengths) if ragged else out


def _is_int(value):
    return isinstance(value, (int, np.integer))


def _per_row(rate, rows, name):
    if isinstance(rate, torch.Tensor):
        if rate.is_cuda:
            raise ValueError(
                f'{name}: per-row rates are given on the host (a list or a '
                'CPU tensor); the table scaling and the output size come '
                'from them')
        rate = rate.reshape(-1).tolist()
    if isinstance(rate, (list, tuple)):
        if len(rate) != rows:
            raise ValueError(f'{len(rate)} values of {name} for {rows} rows')
        return [int(item) for item in rate]
    return [int(rate)] * rows


def _device(flat, lengths, orig, new, n_out):
    """One launch per table scaling over the rows that share it"""
    rows, samples = flat.shape
    device = flat.device
    out = torch.empty(rows, n_out, dtype=torch.float32, device=device)
    if rows == 0 or n_out == 0:
        return out
    if flat.stride(1) != 1 or (rows > 1 and flat.stride(0) < samples):
        flat = flat.contiguous()
    groups = {}
    for row in range(rows):
        groups.setdefault(scaling(orig[row], new[row]), []).append(row)
    with torch.cuda.device(device):
        for scale, members in groups.items():
            win, delta = device_tables(scale, device)
            whole = len(members) == rows
            source = flat if whole else flat[members]
            target = out if whole else torch.empty(
                len(members), n_out, dtype=torch.float32, device=device)
            meta = torch.tensor(
                [[lengths[row] for row in members],
                 [orig[row] for row in members],
                 [new[row] for row in members]],
                dtype=torch.int32).to(device)
            stride = source.stride(0) if len(members) > 1 else samples
            _lib.check(_lib.lib().pm_resample_interp(
                source.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
                meta[2].data_ptr(), _lib.ptr(win), _lib.ptr(delta),
                target.data_ptr(), len(members), samples,
                max(stride, samples), n_out, n_out, _lib.stream()))
            if not whole:
                out[members] = target
    return out


###############################################################################
# The host path
###############################################################################


def _fma32(a, b, c):
    """round_to_fp32(a b + c) of fp32 arrays with ONE rounding: the product of
    two 24-bit significands is exact in float64, the sum is rounded to odd
    there (the residual of TwoSum says which way), and 53 >= 24 + 2 bits make
    the final rounding the one an fp32 fma takes."""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64)
               for t in (a, b, c))
    product = a * b
    total = product + c
    virtual = total - product
    residual = (product - (total - virtual)) + (c - virtual)
    even = (total.view(np.int64) & 1) == 0
    toward = np.where(residual > 0, np.inf, -np.inf)
    odd = np.where((residual != 0) & even, np.nextafter(total, toward), total)
    return odd.astype(np.float32)


def host_row(x, orig, new, win, delta):
    """The contract of pm_resample_interp for one row x (length,): fp32
    (length * new // orig,), every output its own fma chain, left wing then
    right wing, ascending."""
    x = np.asarray(x, dtype=np.float32)
    length = x.shape[0]
    n_win = win.shape[0]
    t = np.arange(length * new // orig, dtype=np.int64)
    n, rem = t * orig // new, t * orig % new
    D = max(orig, new)
    step = min(orig, new) * STEPS // orig
    acc = np.zeros(t.shape[0], dtype=np.float32)
    padded = np.concatenate([x, np.zeros(1, np.float32)])
    for scaled, count, first, direction in (
            (rem * STEPS, n + 1, n, -1),
            ((new - rem) * STEPS, length - n - 1, n + 1, 1)):
        off = scaled // D
        eta = (scaled % D).astype(np.float32) / np.float32(D)
        count = np.minimum(count, (n_win - off) // step)
        for i in range(int(count.max(initial=0))):
            live = i < count
            at = np.where(live, off + i * step, 0)
            weight = _fma32(eta, delta[at], win[at])
            sample = padded[np.where(live, first + direction * i, length)]
            acc = np.where(live, _fma32(weight, sample, acc), acc)
    return acc
