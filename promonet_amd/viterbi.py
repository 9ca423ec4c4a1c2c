"""Batched Viterbi decoding on the device (pm_viterbi).

`from_probabilities` has the signature of `torbi.from_probabilities` minus
`gpu` and `num_threads`: torbi is what promonet/preprocess/harmonics.py:270-276
decodes with, and what `penn` decodes the pitch contour with.

Semantics, with A = log transition, B = log observation, p = log initial:

    d_0[j] = B[0, j] + p[j]
    m_t[j] = the i that maximises d_{t-1}[i] + A[j, i]            (t >= 1)
    d_t[j] = B[t, j] + (d_{t-1}[m] + A[j, m])

every sum one fp32 add in that association. The last state is the argmax of
d_{len-1}; earlier states follow the back-pointers. Ties go to the lowest
index in both maxima, the tie of all -inf included. The result is a pure
function of the three fp32 inputs and equals the CPU oracle
(tests/harmonics_oracle.py) exactly. Inputs must be free of NaN and +inf.

`transition[j, i]` is the step FROM i TO j: the row is the next state. To our
knowledge torbi's reference implementation reads it this way
(`posterior[t-1] + transition`, argmax over the last axis), but torbi is not
a dependency and is not installed where this was written: parity with torbi
itself is unpinned.

The kernel reads the transition banded (`Transition`): for every next state
the range that holds all its finite entries. The band is packed once per
matrix with torch ops and kept, by the caller in a `Transition` or here in a
small cache keyed on the tensor's storage and version.
"""
import weakref

import torch

import promonet_amd


class Transition:
    """The banded log transition the kernel reads.

    table (3, S) int32: lo, count, offset of every next state j;
    band[offset_j + k] = A[j, lo_j + k] for k < count_j, padded with -inf to
    a multiple of 4 floats. [lo_j, lo_j + count_j) contains every finite
    A[j, .]; -inf inside it stays -inf; a dense matrix is the band [0, S)."""

    def __init__(self, transition, log_probs=False):
        if transition.ndim != 2 or transition.shape[0] != transition.shape[1]:
            raise ValueError(
                f'transition must be (states, states), got '
                f'{tuple(transition.shape)}')
        log = transition.to(torch.float32)
        if not log_probs:
            log = torch.log(log)
        self.states = log.shape[0]
        self.table, self.band = pack_band(log)

    def dense(self):
        """The (states, states) log transition the band stands for"""
        return unpack_band(self.table, self.band)

    def to(self, device):
        moved = object.__new__(Transition)
        moved.states = self.states
        moved.table, moved.band = self.table.to(device), self.band.to(device)
        return moved


def pack_band(log_transition):
    """(table (3, S) int32, band float32) of a log transition (S, S), on its
    device, with torch ops only"""
    states = log_transition.shape[0]
    device = log_transition.device
    finite = log_transition > -float('inf')
    index = torch.arange(states, device=device)
    any_finite = finite.any(dim=1)
    first = torch.where(finite, index[None], states).amin(dim=1)
    last = torch.where(finite, index[None], -1).amax(dim=1)
    lo = torch.where(any_finite, first, 0)
    count = torch.where(any_finite, last + 1 - first, 0)
    padded = (count + 3) // 4 * 4
    offset = torch.cumsum(padded, 0) - padded
    total = int(padded.sum())
    if total >= 2 ** 31:
        raise ValueError(f'a band of {total} floats is too large')
    rows = torch.repeat_interleave(index, padded)
    within = torch.arange(total, device=device) - offset[rows]
    columns = lo[rows] + within
    inside = within < count[rows]
    values = log_transition[rows, columns.clamp(max=states - 1)]
    band = torch.where(inside, values, -float('inf')).to(torch.float32)
    table = torch.stack([lo, count, offset]).to(torch.int32).contiguous()
    return table, band.contiguous()


def unpack_band(table, band):
    """The dense log transition (S, S) of a packed band: the inverse of
    `pack_band`"""
    lo, count, offset = (item.to(torch.int64) for item in table)
    states = lo.numel()
    index = torch.arange(states, device=band.device)
    within = index[None] - lo[:, None]
    inside = (within >= 0) & (within < count[:, None])
    position = (offset[:, None] + within).clamp(0, max(band.numel() - 1, 0))
    if band.numel() == 0:
        return torch.full(
            (states, states), -float('inf'), device=band.device)
    return torch.where(inside, band[position], -float('inf'))


# (S + 7) // 4 * 4 floats a row of scores, two rows in 64 KiB (pm_viterbi.h)
MAX_STATES = 8188

_bands = {}
BAND_CACHE_SIZE = 8


def banded(transition, log_probs=False):
    """The `Transition` of a tensor, packed once per (storage, version)"""
    if isinstance(transition, Transition):
        return transition
    key = (transition.data_ptr(), transition._version,
           tuple(transition.shape), tuple(transition.stride()),
           transition.dtype, str(transition.device), bool(log_probs))
    entry = _bands.get(key)
    if entry is not None and entry[0]() is transition:
        return entry[1]
    packed = Transition(transition, log_probs)
    if len(_bands) >= BAND_CACHE_SIZE:
        _bands.pop(next(iter(_bands)))
    _bands[key] = (weakref.ref(transition), packed)
    return packed


_uniform = {}


def uniform(states, device):
    """torbi's defaults: (Transition, log initial) of the uniform
    distributions, log(1 / states) in fp32 everywhere"""
    key = (states, str(device))
    if key not in _uniform:
        value = torch.log(torch.full(
            (states,), 1. / states, dtype=torch.float32, device=device))
        table = torch.stack([
            torch.zeros(states, dtype=torch.int64),
            torch.full((states,), states),
            torch.arange(states) * ((states + 3) // 4 * 4)]).to(torch.int32)
        row = torch.full(
            ((states + 3) // 4 * 4,), -float('inf'), device=device)
        row[:states] = value
        packed = object.__new__(Transition)
        packed.states = states
        packed.table = table.to(device)
        packed.band = row.repeat(states).contiguous()
        _uniform[key] = (packed, value)
    return _uniform[key]


def from_probabilities(
    observation,
    batch_frames=None,
    transition=None,
    initial=None,
    log_probs=False
):
    """Decode a batch of time-varying categorical distributions

    Arguments
        observation
            shape=(batch, frames, states) float32, on the device
        batch_frames
            Frames of each row: a list or a tensor; None: all of them
        transition
            (states, states) tensor or a `Transition`; transition[j, i] is
            the step from i to j; None: uniform
        initial
            (states,); None: uniform
        log_probs
            Whether observation, transition and initial are log-probabilities

    Returns
        indices: int32 (batch, frames) on the device, 0 past a row's frames
    """
    _lib = promonet_amd._lib
    _lib.require_gpu(observation)
    if observation.ndim != 3:
        raise ValueError(
            'observation must be (batch, frames, states), got '
            f'{tuple(observation.shape)}')
    if observation.dtype != torch.float32:
        raise RuntimeError(f'expected torch.float32, got {observation.dtype}')
    device = observation.device
    batch, frames, states = observation.shape
    if states < 1:
        raise ValueError('observation has no states')
    if states > MAX_STATES:
        raise ValueError(
            f'{states} states: the kernel keeps two rows of scores in 64 KiB '
            f'of LDS and int16 back-pointers, at most {MAX_STATES} states')
    if not log_probs:
        observation = torch.log(observation)
    observation = observation.contiguous()
    if transition is None:
        band = uniform(states, device)[0]
    else:
        if not isinstance(transition, Transition):
            _lib.require_gpu(transition)
        band = banded(transition, log_probs)
    if band.states != states:
        raise ValueError(
            f'transition has {band.states} states, observation {states}')
    if initial is None:
        initial = uniform(states, device)[1]
    else:
        _lib.require_gpu(initial)
        if initial.shape != (states,):
            raise ValueError(
                f'initial must be ({states},), got {tuple(initial.shape)}')
        initial = initial.to(torch.float32)
        if not log_probs:
            initial = torch.log(initial)
        initial = initial.contiguous()
    lengths = None
    if batch_frames is not None:
        if isinstance(batch_frames, (list, tuple)):
            batch_frames = torch.tensor(batch_frames, dtype=torch.int32)
        if batch_frames.numel() != batch:
            raise ValueError(
                f'{batch_frames.numel()} lengths for {batch} rows')
        lengths = batch_frames.reshape(-1).to(
            device=device, dtype=torch.int32).contiguous()
    out = torch.empty(batch, frames, dtype=torch.int32, device=device)
    if batch == 0 or frames == 0:
        return out
    library = _lib.lib()
    size = library.pm_viterbi_workspace(batch, frames, states)
    workspace = torch.empty(max(size, 1), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(library.pm_viterbi(
            _lib.ptr(observation),
            _lib.ptr(lengths, torch.int32),
            _lib.ptr(band.band),
            band.band.numel(),
            _lib.ptr(band.table, torch.int32),
            _lib.ptr(initial),
            _lib.ptr(out, torch.int32),
            batch, frames, states,
            workspace.data_ptr(), workspace.numel(), _lib.stream()))
    return out
