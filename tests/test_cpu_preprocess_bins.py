"""The oracle of the preprocessing transforms (tests/preprocess_oracle.py) on
the CPU: its case table has the geometry it is named for, the recorded fp32
figures are what torch.stft reaches on the common MKL path (GATES, to 2 %;
K = 4 x), every
planted defect is rejected by some case at K, and the older flat gates on
white noise accept several of them - the statement of what
tests/test_gpu_preprocess_bins.py adds.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import preprocess_oracle as oracle
import restatement as R

# the cases the planted defects are run on (a 512 x 512 float64 DFT a frame)
DEFECT_CASES = (
    'noise', 'impulses', 'cosines', 'cosines_floor', 'levels', 'length_385',
    'frames_17')


def test_case_table_shapes():
    cases = oracle.cases()
    assert cases['cosines'].shape == (12, 2049)
    assert cases['impulses'].shape == (5, 2048)
    for samples in oracle.LENGTHS:
        assert cases[f'length_{samples}'].shape == (3, samples)
    for frames in oracle.FRAME_COUNTS:
        audio = cases[f'frames_{frames}']
        assert audio.shape[0] == 2 and audio.shape[1] // 256 == frames
        assert audio.shape[1] % 2 == 1       # row 1 on the unaligned load
    # the tail of the 16-byte row store at nf % 4 = 1, 2, 3, a last group of
    # one frame at both group sizes, odd T
    for per_group in (16, 32):
        tails = {(frames - 1) % per_group + 1 for frames in oracle.FRAME_COUNTS}
        assert {tail % 4 for tail in tails} == {0, 1, 2, 3}
        assert 1 in tails
    assert min(oracle.LENGTHS) == oracle.PAD + 1
    for name, audio in cases.items():
        t = oracle.case_truth(name)
        assert t['magnitude'].shape == (
            audio.shape[0], 513, audio.shape[1] // 256), name
        assert audio.dtype == torch.float32 and torch.isfinite(audio).all()


def test_each_cosine_has_three_bins():
    """In float64, before the samples are rounded: bins k - 1, k, k + 1 and
    nothing else (two bins at k = 0 and k = 512), in every frame - both
    reflections continue the cosine"""
    x = oracle.model_bins(oracle.cosines(torch.float64).numpy())
    assert x.shape == (12, 513, 8)
    for row, k in enumerate(oracle.COSINE_BINS):
        occupied = (x[row] > 1e-9).all(1)
        empty = (x[row] < 1e-9).all(1)
        assert (occupied | empty).all()
        want = [b for b in (k - 1, k, k + 1) if 0 <= b <= 512]
        assert occupied.nonzero().flatten().tolist() == want
        peak = 256. if k in (0, 512) else 128.
        assert (x[row, k] - peak).abs().max() < 1e-9
        assert len(want) == (2 if k in (0, 512) else 3)


def test_impulse_bins_are_the_window():
    """A frame that sees one unit sample has |X_k| = the window's value
    there, for every k"""
    t = oracle.case_truth('impulses')
    hann = torch.hann_window(1024, dtype=torch.float64)
    frames = oracle.model_frames(oracle.cases()['impulses'].double().numpy())
    copies = (frames != 0).sum(-1)                  # (rows, frames)
    # in a reflection a sample is seen twice; sample 0 and the last one are
    # reflected onto themselves: seen once
    assert copies[0].max() == 2 and copies[3].max() == 2
    assert copies[[1, 2, 4]].max() == 1
    for row in range(5):
        once = np.nonzero(copies[row] == 1)[0]
        assert len(once), row
        for frame in once:
            n = int(frames[row, frame].argmax())
            assert (t['x'][row, :, frame] - hann[n]).abs().max() < 1e-9
    # frame 0 of row 0: two copies beat across the bins
    assert (t['x'][0, :, 0].max() - t['x'][0, :, 0].min()) > .1


def test_floor_shares_and_silence():
    for name in ['cosines_floor'] + [
            f'frames_{frames}' for frames in oracle.FRAME_COUNTS]:
        under, over = oracle.floor_shares(oracle.case_truth(name))
        assert under >= .2 and over >= .2, (name, under, over)
    t = oracle.case_truth('levels')
    assert (t['db'][0] == oracle.MIN_DB).all()               # silence
    for bands in (8, 1, 3, 16):
        assert (R.band_average(t['db'], bands)[0] == oracle.MIN_DB).all()
    # the rows keep their own floors: 60 dB apart
    floors = t['floor'].flatten()
    assert abs(floors[3] - floors[4] - 60.) < 1e-3
    # sub-clamp noise: bins on both sides of the 1e-5 amplitude clamp
    assert (t['x'][1] < 1e-5).any() and (t['x'][1] > 1e-5).any()
    assert oracle.cases()['levels'][2].abs().min() == 1.
    for side, name in ((+1, 'floor_above'), (-1, 'floor_below')):
        t = oracle.case_truth(name)
        minimum = t['raw_db'][0, :, :16].min().item()
        assert abs(minimum + 100.) < 1e-9
        assert 0 < side * (t['floor'].item() - minimum) < 1e-3


def test_the_kernel_algebra_is_the_contract():
    """The packed 512-point transform and its unpacking (oracle.model_bins,
    the form that takes the planted defects) against the restatement"""
    for name in DEFECT_CASES:
        figures = oracle.model_figures(name)
        assert figures['magnitude'] < 1e-6 and figures['log_mel'] < 1e-6
        # (the dB truth is rounded to float32 by the restatement)
        assert figures['db_bin'] < .26 and figures['band_mean'] < .05
        t = oracle.case_truth(name)
        x = oracle.model_bins(oracle.cases()[name].double().numpy())
        assert (x - t['x']).abs().max() < 1e-9
        frames = oracle.model_frames(oracle.cases()[name].double().numpy())
        l2 = np.sqrt(((frames * oracle.model_tables()[0]) ** 2).sum(-1))
        assert np.abs(l2 - t['l2'][:, 0].numpy()).max() < 1e-9


def test_gates_are_four_times_the_fp32_figures():
    """MKL chooses its transform by the processor, so the figures are taken
    in a child process on the code path that every processor has"""
    root = Path(__file__).resolve().parent
    script = (
        'import json, sys\n'
        f'sys.path[:0] = [{str(root)!r}, {str(root.parent / "oracle")!r}]\n'
        'import preprocess_oracle as oracle\n'
        'print(json.dumps({name: oracle.fp32_figures(name) '
        'for name in oracle.cases()}))\n')
    environment = dict(
        os.environ, MKL_CBWR='COMPATIBLE', OMP_NUM_THREADS='1',
        MKL_NUM_THREADS='1')
    output = subprocess.run(
        [sys.executable, '-c', script], env=environment, check=True,
        capture_output=True, text=True).stdout
    table = json.loads(output.splitlines()[-1])
    assert list(table) == list(oracle.cases())
    largest, where = {}, {}
    for name, figures in table.items():
        print(name + ': ' + ', '.join(
            f'{family} {figures[family]:.3f}' for family in oracle.FAMILIES))
        for family, value in figures.items():
            if value > largest.get(family, 0.):
                largest[family], where[family] = value, name
    print('largest:', largest, where)
    for family in oracle.FAMILIES:
        assert abs(largest[family] / oracle.GATES[family] - 1.) < .02, family
        assert oracle.K[family] == 4. * oracle.GATES[family]
    # whatever path this process takes, its figures are within the gates
    for name in ('cosines', 'cosines_floor', 'frames_35', 'impulses'):
        here = oracle.fp32_figures(name)
        print(f'in this process, {name}:', here)
        for family, value in here.items():
            assert 0 <= value < oracle.K[family]


@pytest.fixture(scope='module')
def defect_figures():
    """{defect: {family: (largest figure, its case)}}"""
    out = {}
    for defect in oracle.DEFECTS:
        best = {}
        for name in DEFECT_CASES:
            for family, value in oracle.model_figures(name, defect).items():
                if value > best.get(family, (0., None))[0]:
                    best[family] = (value, name)
        out[defect] = best
    return out


@pytest.mark.parametrize('defect', oracle.DEFECTS)
def test_planted_defect_is_rejected(defect_figures, defect):
    best = defect_figures[defect]
    rejected = {family: (round(value, 2), name)
                for family, (value, name) in best.items()
                if value >= oracle.K[family]}
    print(defect, 'rejected by', rejected)
    assert rejected, (defect, best)


def old_gate_ratio(got, want, gate):
    return ((got - want).abs() / (gate[0] + gate[1] * want.abs())).max().item()


def test_blind_spots_of_the_flat_gates():
    """What 2e-5 + 1e-5 |want| (magnitude, log-mel) and 1e-4 dB + 1e-5 |want|
    (the band means) on white noise at 0.1 - all that the older tests hold -
    accept, and the per-bin models do not"""
    audio = oracle.cases()['noise'].double().numpy()
    t = oracle.case_truth('noise')
    accepted = []
    for defect in oracle.DEFECTS:
        out = oracle.model_outputs(audio, defect)
        worst = max(
            old_gate_ratio(out['magnitude'], t['magnitude'],
                           oracle.OLD_STFT_GATE),
            old_gate_ratio(out['log_mel'], t['log_mel'], oracle.OLD_STFT_GATE),
            old_gate_ratio(out['bands'][8], R.band_average(t['db'], 8),
                           oracle.OLD_LOUDNESS_GATE))
        # (per bin the older tests add a conditioning allowance for weak bins
        # to the flat gate, test_gpu_preprocess_full.py: printed, not counted)
        per_bin = old_gate_ratio(out['db'], t['db'], oracle.OLD_LOUDNESS_GATE)
        print(f'{defect}: worst error over the flat gates {worst:.3f} '
              f'(dB per bin {per_bin:.3f})')
        if worst < 1.:
            accepted.append(defect)
    print('accepted by the flat gates on white noise:', accepted)
    for defect in ('window_2e-6', 'w1024_2e-6', 'w512_entry'):
        assert defect in accepted
    # weak bins of the sparse cases: every bin that should be ~0 raised by
    # 1e-4 passes the flat gate and misses the model by orders
    t = oracle.case_truth('cosines')
    weak = t['x'] < 1e-6
    assert weak.double().mean() > .9
    raised = ((t['x'] + 1e-4 * weak) ** 2 + 1e-6).sqrt()
    flat = old_gate_ratio(raised, t['magnitude'], oracle.OLD_STFT_GATE)
    print(f'weak bins raised by 1e-4: {flat:.2f} of the flat gate')
    assert flat < 1.
    figure = oracle.figure(raised, t['magnitude'], oracle.magnitude_bound(t))
    print(f'weak bins raised by 1e-4: figure {figure:.0f}')
    assert figure > oracle.K['magnitude']
