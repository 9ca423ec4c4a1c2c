"""The float64 oracle of the Vocos head (tests/vocos_head_oracle.py): its
tables meet the conditions their gates rest on, the recorded fp32 figures
reproduce, the reference's own fp32 arithmetic passes every comparison of
tests/test_gpu_vocos_head.py, and every planted defect fails the comparison
that is meant to catch it. No GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import vocos_head_oracle as oracle


###############################################################################
# The tables meet their own conditions
###############################################################################


def coverage(live, count):
    """How many live frames reach each sample of the uncropped overlap-add"""
    reached = torch.zeros((count - 1) * oracle.HOP + oracle.N_FFT,
                          dtype=torch.int64)
    for entry in live:
        first = entry[1] * oracle.HOP
        reached[first:first + oracle.N_FFT] += 1
    return reached


def test_per_bin_table_has_one_live_frame_a_sample():
    spec, window, live = oracle.per_bin_table()
    assert spec.shape == (2, 513, 4 * 513 + 4) and window.shape == (1024,)
    assert spec.dtype == torch.complex64 and window.dtype == torch.float32
    for row in range(2):
        mine = [entry for entry in live if entry[0] == row]
        assert sorted(entry[2] for entry in mine) == list(range(513))
        reached = coverage(mine, spec.shape[2])
        assert (reached[:1024 * 513] == 1).all()
        assert (reached[1024 * 513:] == 0).all()
    assert live[0] == (0, 0, 0) and live[513] == (1, 0, 512)
    # one bin a live frame, nothing anywhere else
    assert int((spec != 0).sum()) == len(live) == 2 * 513
    for row, frame, k in live:
        value = spec[row, k, frame]
        assert .5 <= abs(value.real) <= 2 and .5 <= abs(value.imag) <= 2
    assert window.min() > 0 and not torch.equal(window, window.flip(0))
    # (the periodic Hann window is its own mirror one sample on)
    assert not torch.equal(window[1:], window.flip(0)[:-1])


@pytest.mark.parametrize('count', oracle.EXACT_FRAMES)
def test_exact_table_is_exact_in_fp32(count):
    spec, window = oracle.exact_table(count)
    assert spec.shape == (oracle.EXACT_BATCH, 513, count)
    ends = spec[:, [0, 512]]
    assert int((spec != 0).sum()) <= ends.numel()
    assert (spec[:, 1:512] == 0).all()
    assert (ends.imag != 0).all()
    assert torch.equal(ends.real, ends.real.round())
    assert ends.real.abs().max() <= 8
    rows = [tuple(row.flatten().tolist()) for row in ends.real]
    assert len(set(rows)) == len(rows)
    if count > 1:
        assert all(len({tuple(frame.tolist()) for frame in row.T}) > 1
                   for row in ends.real)
    m = window.double() * 64
    assert torch.equal(m, m.round()) and m.min() >= 1 and m.max() <= 64
    assert not torch.equal(window, window.flip(0))
    assert not torch.equal(window[1:], window.flip(0)[:-1])
    # every frame sample is an integer in units of 2^-16, at most 16 x 64
    units = oracle.frames(spec, window) * 2. ** 16
    assert torch.equal(units, units.round()) and units.abs().max() <= 1024
    # so a sum of four stays far below 2^24 units, and so does the envelope's
    # in units of 2^-12
    square = window.double().square() * 4096
    assert torch.equal(square, square.round()) and 4 * square.max() < 2 ** 24
    assert 4 * 1024 < 2 ** 24
    # the oracle rounded once is finite, and it is what the reference's own
    # fp32 arithmetic gives
    want = oracle.exact_oracle(count)
    assert want.shape == (oracle.EXACT_BATCH, 256 * count)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(oracle.reference_istft(spec, window), want)


def test_silence_is_exactly_zero_in_fp32():
    assert np.exp(np.float32(oracle.SILENT)) == 0
    assert torch.exp(torch.tensor(oracle.SILENT)).item() == 0
    assert np.float32(np.exp(np.float64(oracle.SILENT))) == 0


@pytest.mark.parametrize('which', oracle.HEAD_SETS)
def test_head_table_is_exact_in_every_operand_type(which):
    x, weight, window, live = oracle.head_table(which)
    assert x.shape == (2, oracle.HEAD_FRAMES, 512) == (2, 2048, 512)
    assert weight.shape == (1026, 512)
    # at most 8 significant bits: bf16 holds 8, f16 11
    assert torch.equal(weight.bfloat16().float(), weight)
    assert torch.equal(weight.half().float(), weight)
    # one-hot rows: the logits are a column of the weight, whatever the order
    # and the type of the products
    assert ((x == 0) | (x == 1)).all() and (x.sum(-1) == 1).all()
    logits = oracle.head_logits(which)
    channel = x.argmax(-1)
    assert torch.equal(logits, weight.T[channel])
    log_magnitude, phase = weight[:513], weight[513:]
    assert (phase != 0).all()
    assert (log_magnitude[:, oracle.SILENT_CHANNEL] == oracle.SILENT).all()
    for row in range(2):
        mine = [entry for entry in live if entry[0] == row]
        reached = coverage(mine, oracle.HEAD_FRAMES)
        assert (reached[:1024 * 511] == 1).all()
        assert (reached[1024 * 511:] == 0).all()
        assert sorted(entry[2] for entry in mine) == list(range(511))
    for row, frame, c, k, value in live:
        assert channel[row, frame] == c
        column = log_magnitude[:, c]
        assert column[k] == value and -6 <= value <= 6
        assert int((column != oracle.SILENT).sum()) == 1
    silent = torch.ones(2, oracle.HEAD_FRAMES, dtype=torch.bool)
    for row, frame, *_ in live:
        silent[row, frame] = False
    assert (channel[silent] == oracle.SILENT_CHANNEL).all()
    # every log-magnitude of the grid, both sides of the clip, large phases
    assert {entry[4] for entry in live} == set(oracle.LOG_MAGNITUDES)
    assert np.exp(4.5) < 100 < np.exp(4.625) < np.exp(5.)
    own = torch.tensor([phase[k, c].item() for _, _, c, k, _ in live])
    assert set(oracle.LARGE_PHASES) <= set(own.tolist())
    assert (own.abs() < 32).sum() > 400
    assert oracle.head_silence(which) == 1024 * 511 - 384


def test_the_two_head_sets_cover_every_bin():
    bins = set()
    for which in oracle.HEAD_SETS:
        bins |= {entry[3] for entry in oracle.head_table(which)[3]}
    assert bins == set(range(513))


###############################################################################
# The gates
###############################################################################


def test_gates_are_four_times_the_recorded_fp32_figures():
    """MKL chooses its transform by the processor, so the figures are taken
    in a child process on the code path that every processor has"""
    script = (
        'import json, sys\n'
        f'sys.path.insert(0, {str(Path(__file__).parent)!r})\n'
        'import vocos_head_oracle as oracle\n'
        'print(json.dumps([oracle.per_bin_fp32_figure(), '
        'oracle.head_fp32_figure()]))\n')
    environment = dict(
        os.environ, MKL_CBWR='COMPATIBLE', OMP_NUM_THREADS='1',
        MKL_NUM_THREADS='1')
    output = subprocess.run(
        [sys.executable, '-c', script], env=environment, check=True,
        capture_output=True, text=True).stdout
    per_bin, head = json.loads(output.splitlines()[-1])
    print(f'fp32 reference: per bin {per_bin:.3e}, head {head:.3e}')
    assert float(f'{per_bin:.3e}') == oracle.PER_BIN_FP32_FIGURE == 1.043e-06
    assert float(f'{head:.3e}') == oracle.HEAD_FP32_FIGURE == 1.029e-06
    assert oracle.PER_BIN_GATE == 4 * oracle.PER_BIN_FP32_FIGURE
    assert oracle.HEAD_GATE == 4 * oracle.HEAD_FP32_FIGURE


def test_the_reference_fp32_arithmetic_passes_every_gate():
    """Whatever path this process takes"""
    here = oracle.per_bin_fp32_figure()
    print(f'per bin, in this process: {here:.3e}')
    assert 0 < here < oracle.PER_BIN_GATE
    here = oracle.head_fp32_figure()
    print(f'head, in this process: {here:.3e}')
    assert 0 < here < oracle.HEAD_GATE
    for which in oracle.HEAD_SETS:
        _, _, window, live = oracle.head_table(which)
        got = reference_head(which)
        assert (got[:, oracle.head_silence(which):] == 0).all()
        for value in oracle.CLIP_SIDES:
            assert 0 < clip_side(got, which, value) < oracle.HEAD_GATE


###############################################################################
# Every planted defect fails the comparison meant to catch it
###############################################################################


_reference = {}


def reference_head(which):
    if which not in _reference:
        _reference[which] = oracle.reference_head(
            oracle.head_logits(which), oracle.head_table(which)[2])
    return _reference[which]


def clip_side(got, which, value, defect=None):
    """The figure of the live frames whose log-magnitude is `value`"""
    live = [entry for entry in oracle.head_table(which)[3]
            if entry[4] == value]
    assert len(live) >= 10
    return oracle.figure(got, oracle.head_oracle(which), live)[0]


def accepted_per_bin(defect):
    spec, window, live = oracle.per_bin_table()
    got = oracle.istft(spec, window, defect)
    return oracle.figure(got, oracle.per_bin_oracle(), live)[0] < \
        oracle.PER_BIN_GATE


def accepted_exact(defect):
    """Per frame count: the fp32 outputs are equal"""
    return [torch.equal(oracle.exact_oracle(count, defect),
                        oracle.exact_oracle(count))
            for count in oracle.EXACT_FRAMES]


def accepted_head(defect):
    """Per weight set"""
    result = []
    for which in oracle.HEAD_SETS:
        live = oracle.head_table(which)[3]
        got = oracle.head_oracle(which, defect)
        result.append(oracle.figure(got, oracle.head_oracle(which), live)[0] <
                      oracle.HEAD_GATE)
    return result


# defect -> the comparisons that must reject it
APPLIES = {
    'imag_dc_kept': ('per bin', 'exact'),
    'imag_nyquist_kept': ('per bin', 'exact'),
    'image_not_conjugated': ('per bin', 'head'),
    'window_mirrored': ('per bin', 'exact'),
    'crop_383': ('per bin', 'exact', 'head'),
    # (the last 384 samples are silent in the per-bin and the head tables)
    'envelope_unclamped': ('exact',),
    'clip_before_exp': ('head',),
    'clip_at_10': ('head',),
}


def test_the_defects_are_all_listed():
    assert set(APPLIES) == set(oracle.DEFECTS)


def test_the_oracle_itself_is_accepted():
    assert accepted_per_bin(None)
    assert all(accepted_exact(None))
    assert all(accepted_head(None))


@pytest.mark.parametrize(
    'defect,comparison',
    [(defect, comparison) for defect in oracle.DEFECTS
     for comparison in APPLIES[defect]])
def test_a_planted_defect_is_rejected(defect, comparison):
    if comparison == 'per bin':
        assert not accepted_per_bin(defect)
    elif comparison == 'exact':
        # at every frame count, T = 1 included
        assert not any(accepted_exact(defect))
    else:
        # in either weight set
        assert not any(accepted_head(defect))


def test_a_defect_is_seen_at_the_bin_it_sits_in():
    """The figure is per frame, so it names the bin"""
    spec, window, live = oracle.per_bin_table()
    want = oracle.per_bin_oracle()
    for defect, k in (('imag_dc_kept', 0), ('imag_nyquist_kept', 512)):
        got = oracle.istft(spec, window, defect)
        for row in range(2):
            mine = [entry for entry in live if entry[0] == row]
            worst, where = oracle.figure(got, want, mine)
            assert where[2] == k and worst > .1
            others = [entry for entry in mine if entry[2] != k]
            assert oracle.figure(got, want, others)[0] == 0


@pytest.mark.parametrize('which', oracle.HEAD_SETS)
def test_the_clip_shows_on_either_side(which):
    """The amplitudes with and without the clip differ by far more than the
    gate: e^4.5 = 90 against 10, 100 against e^4.625 = 102 and e^5 = 148"""
    for value, defect, least in ((4.5, 'clip_at_10', .8),
                                 (4.625, 'clip_before_exp', .02),
                                 (5., 'clip_before_exp', .4)):
        got = oracle.head_oracle(which, defect)
        figure = clip_side(got, which, value)
        print(f'{which} {value} {defect}: {figure:.3e}')
        assert figure > least > 1000 * oracle.HEAD_GATE
    # e^4.5 is below the clip: clipping before the exp leaves it alone
    assert clip_side(oracle.head_oracle(which, 'clip_before_exp'), which,
                     4.5) == 0
