"""Every case of test_gpu_out_rows.py is built here, without a GPU, and is
inside the exact range: at most E.EXACT_BITS bits of bound / quantum, the
result a fixed point of a round trip through fp32 (exact_oracle.exactness
raises otherwise). A chosen input that leaves the range fails here instead of
going unnoticed on a machine that skips the GPU file."""
import pytest
import torch

import exact_oracle as E
import out_rows_cases as R


@pytest.mark.parametrize('mode,k,d,length', R.pair_table())
def test_pair_case_is_exact(mode, k, d, length):
    case = R.pair_case(mode, k, d, length)
    assert 0 < case['bits'] <= E.EXACT_BITS, case['bits']
    for want in case['want'].values():
        assert torch.equal(want.float().double(), want)


@pytest.mark.parametrize('mode', R.MODES)
def test_ragged_pair_case_is_exact(mode):
    length = max(R.PAIR_RAGGED)
    for b, valid in enumerate(R.PAIR_RAGGED):
        alone = R.pair_alone(mode, 11, 5, length, b, valid)
        assert 0 < alone['bits'] <= E.EXACT_BITS, alone['bits']


@pytest.mark.parametrize('c,k,form,index', R.block_table())
def test_block_case_is_exact(c, k, form, index):
    case = R.block_case(c, k, form, index)
    assert 0 < case['bits'] <= E.EXACT_BITS, case['bits']
    assert case['store_mode'] in (1, 2)
    assert torch.equal(case['want'].float().double(), case['want'])


def test_block_cases_cover_the_conditions():
    """Store modes 1 and 2, act16 as bf16 and as f16, 1, 2 and 3 forced
    segments, and the three lengths, for every shape they apply to"""
    for c, k, form, _ in R.BLOCK_SHAPES:
        runs = R.block_runs(c, k, form)
        assert {r[5] for r in runs} == {1, 2}
        assert {r[4] for r in runs} == set(R.block_lengths(c))
        if form == 'skewed':
            assert {r[6] for r in runs} == {None, 'bf16', 'f16'}
        if form != 'tiled':
            assert {r[3] for r in runs} == {1, 2, 3}


@pytest.mark.parametrize('index', range(len(R.MRF_RUNS)))
def test_mrf_case_is_exact(index):
    case = R.mrf_case(index)
    assert 0 < case['bits'] <= E.EXACT_BITS, case['bits']
