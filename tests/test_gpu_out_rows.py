"""The Block kernels' `out` stores, exactly: `torch.equal` with the float64
oracle of exact_oracle.py, no tolerance.

With 16-bit operands a wave turns its 32-column accumulator tiles round in
LDS and stores - and, accumulating, first loads - whole lines of `out`
(pm_store_out_rows, pm_conv.h): conv_pair_kernel in the dead `inter` tile,
block3_body (the tiled and walked whole-Block kernels, the whole-MRF ones) in
the dead `a` tile, the skewed whole-Block walk in the dead `t` tile, where it
also writes the 16-bit operand copy `act16`. A store that lands in the wrong
row, column or channel, that is dropped, that goes past an utterance's or a
segment's end, or an old value read from the wrong place, shows as whole units
of the value grid (out_rows_cases.py: small integers, every sum exact and
independent of its order). `out` starts as a sentinel; in store mode 2 as
integers of the value grid.

The whole MRF (C = 32) holds the exact sum S of its three Blocks in registers
and scales it once, by the host's fp32 1.f / 3.f: the stored value is
fp32(S * fp32(1 / 3)), one correctly rounded product, which float64 reproduces
(22 + 24 bits, then one rounding) - `torch.equal` there too.
"""
import ctypes

import pytest
import torch

import exact_oracle as E
import out_rows_cases as R
from util import from_cl, pad32, to_cl

pytestmark = pytest.mark.gpu

HALF = {'f16': torch.float16, 'bf16': torch.bfloat16}
SENTINEL = -12345.


def lib():
    from promonet_amd import _lib
    return _lib


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def restore_hooks():
    _lib = lib()
    _lib.check(_lib.lib().pm_debug_force(0, 0))
    _lib.check(_lib.lib().pm_debug_skew(0))


def assert_equal(got, want, detail):
    got = got.double().cpu()
    assert torch.equal(got, want), (detail, E.first_difference(got, want))


def start_of(case, store_mode, device):
    """What `out` holds before the launch, channels-last"""
    if store_mode == 2:
        return to_cl(case['prev']).to(device)
    b, c, length = case['x'].shape
    return torch.full((b, length, pad32(c)), SENTINEL, device=device)


# ---------------------------------------------------------------------------
# (a) conv_pair_kernel
# ---------------------------------------------------------------------------
class PairRunner:
    def __init__(self, device, mode, k):
        _lib = lib()
        self.device, self.mode, self.k = device, mode, k
        size = _lib.lib().pm_op_workspace_bytes(R.PAIR_C, R.PAIR_C, k)
        self.ws = torch.empty(size, dtype=torch.uint8, device=device)

    def __call__(self, x_cl, out, w, d, store_mode, lengths=None):
        _lib = lib()
        batch, length, _ = x_cl.shape
        head = [_lib.DTYPES[self.mode], _lib.ptr(x_cl), _lib.ptr(out),
                *[_lib.ptr(t) for t in w]]
        tail = [batch, length, R.PAIR_C, self.k, d, store_mode,
                E.SCALES[store_mode], self.ws.data_ptr(), self.ws.numel(),
                _lib.stream()]
        if lengths is None:
            _lib.check(_lib.lib().pm_block_iteration_cl(*head, *tail))
        else:
            _lib.check(_lib.lib().pm_block_iteration_ragged_cl(
                *head, lengths.data_ptr(), *tail))
        torch.cuda.synchronize()
        return out


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('k', sorted(R.PAIR_LENGTHS))
def test_pair(device, mode, k):
    """Both geometries: the batch of two (two tiles a wave), and 75 copies
    of it (six tiles a wave; compared on the device, copy by copy)"""
    run = PairRunner(device, mode, k)
    for d in R.PAIR_DILATIONS:
        for length in R.PAIR_LENGTHS[k]:
            case = R.pair_case(mode, k, d, length)
            assert case['bits'] <= E.EXACT_BITS, case['bits']
            w = [t.to(device).contiguous() for t in case['w']]
            x_cl = to_cl(case['x']).to(device)
            many = x_cl.repeat(R.PAIR_REPLICAS, 1, 1)
            for store_mode in R.STORE_MODES:
                detail = (d, length, store_mode)
                want = case['want'][store_mode]
                start = start_of(case, store_mode, device)
                out = run(x_cl, start.clone(), w, d, store_mode)
                assert_equal(from_cl(out, R.PAIR_C), want, detail)
                wide = run(many, start.repeat(R.PAIR_REPLICAS, 1, 1), w, d,
                           store_mode)
                want_cl = to_cl(want).float().to(device)
                copies = wide.view(R.PAIR_REPLICAS, *want_cl.shape)
                same = (copies == want_cl).flatten(1).all(1)
                if not same.all():
                    r = int((~same).nonzero()[0])
                    assert_equal(from_cl(copies[r], R.PAIR_C), want,
                                 (*detail, 'copy', r))


@pytest.mark.parametrize('replicas', (1, R.PAIR_REPLICAS))
@pytest.mark.parametrize('store_mode', (1, 2))
@pytest.mark.parametrize('mode', R.MODES)
def test_pair_ragged(device, mode, store_mode, replicas):
    """Each utterance equals itself alone, and `out` is untouched past its
    end: the sentinel, or in mode 2 the integers it held"""
    k, d, length = 11, 5, max(R.PAIR_RAGGED)
    case = R.pair_case(mode, k, d, length)
    assert case['bits'] <= E.EXACT_BITS, case['bits']
    run = PairRunner(device, mode, k)
    w = [t.to(device).contiguous() for t in case['w']]
    x_cl = to_cl(case['x']).to(device).repeat(replicas, 1, 1)
    start = start_of(case, store_mode, device).repeat(replicas, 1, 1)
    lengths = torch.tensor(R.PAIR_RAGGED * replicas, dtype=torch.int32,
                           device=device)
    out = run(x_cl, start.clone(), w, d, store_mode, lengths)
    for b, valid in enumerate(R.PAIR_RAGGED):
        alone = R.pair_alone(mode, k, d, length, b, valid)
        assert alone['bits'] <= E.EXACT_BITS, alone['bits']
        for r in {0, replicas - 1}:
            at = 2 * r + b
            assert_equal(from_cl(out[at:at + 1, :valid], R.PAIR_C),
                         alone['want'][store_mode], (b, valid, r))
        rows = slice(b, None, 2)
        assert torch.equal(out[rows, valid:], start[rows, valid:]), (b, valid)


# ---------------------------------------------------------------------------
# (b) whole Blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('c,k,form,index', R.block_table())
def test_block(device, c, k, form, index):
    _lib = lib()
    case = R.block_case(c, k, form, index)
    assert case['bits'] <= E.EXACT_BITS, case['bits']
    mode, act, store_mode = case['mode'], case['act'], case['store_mode']
    weights = 3 * _lib.lib().pm_op_workspace_bytes(c, c, k)
    scratch = _lib.lib().pm_walk_scratch_bytes(E.BATCH)
    assert scratch > 0
    ws = torch.empty(weights + (scratch if form == 'skewed' else 0),
                     dtype=torch.uint8, device=device)
    ws[weights:].fill_(0xff)        # (NaNs: nothing stale is read)
    x_cl = to_cl(case['x']).to(device)
    start = start_of(case, store_mode, device)
    out = start.clone()
    w = [[t.to(device).contiguous() for t in ts] for ts in case['w']]
    dil = (ctypes.c_int * len(case['dilations']))(*case['dilations'])
    args = [*[pointers(ts) for ts in w], dil, len(case['dilations']), E.BATCH,
            case['length'], c, k, store_mode, E.SCALES[store_mode],
            ws.data_ptr(), ws.numel(), _lib.stream()]
    detail = (case['nseg'], case['length'], case['dilations'], store_mode, act)
    try:
        _lib.check(_lib.lib().pm_debug_force(case['nseg'], 0))
        _lib.check(_lib.lib().pm_debug_skew(
            {'tiled': 0, 'walked': -1, 'skewed': 1}[form]))
        if act is None:
            _lib.check(_lib.lib().pm_block_cl(
                _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out), *args))
            torch.cuda.synchronize()
            assert_equal(from_cl(out, c), case['want'], detail)
        else:
            act16 = torch.full((E.BATCH, case['length'], pad32(c)), 0x7fff,
                               dtype=torch.int16, device=device)
            _lib.check(_lib.lib().pm_block_act16_cl(
                _lib.DTYPES[mode], _lib.DTYPES[act], _lib.ptr(x_cl),
                _lib.ptr(out), act16.data_ptr(), *args))
            torch.cuda.synchronize()
            # `out` is read (mode 2), never written
            assert torch.equal(out, start), detail
            operand = E.round_operand(
                E.lrelu32(case['want'].float()), act, 'act')
            want = to_cl(operand).to(HALF[act]).view(torch.int16)
            assert torch.equal(act16.cpu(), want), detail
    finally:
        restore_hooks()


# ---------------------------------------------------------------------------
# (c) the whole MRF at C = 32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('nseg', R.MRF_SEGMENTS)
@pytest.mark.parametrize('index', range(len(R.MRF_RUNS)))
def test_mrf(device, index, nseg):
    """out = fp32(S * fp32(1 / 3)): S exact, one scaling, one rounding. (One
    and two iterations take conv_mrf_kernel, forced segments or not: the
    walked whole-MRF kernel exists for three, which no input makes exact.)"""
    _lib = lib()
    case = R.mrf_case(index)
    assert case['bits'] <= E.EXACT_BITS, case['bits']
    c, niter, length = R.MRF_C, case['niter'], R.MRF_LENGTH
    weights = 3 * niter * _lib.lib().pm_op_workspace_bytes(c, c, 11)
    ws = torch.empty(weights, dtype=torch.uint8, device=device)
    x_cl = to_cl(case['x']).to(device)
    order = [[t.to(device).contiguous()
              for block in case['blocks'] for t in block[which]]
             for which in range(4)]
    dil = (ctypes.c_int * niter)(*case['dilations'])
    out = torch.full_like(x_cl, SENTINEL)
    try:
        _lib.check(_lib.lib().pm_debug_force(nseg, 0))
        _lib.check(_lib.lib().pm_mrf_cl(
            _lib.DTYPES[case['mode']], _lib.ptr(x_cl), _lib.ptr(out),
            *[pointers(ts) for ts in order], dil, niter, E.BATCH, length, c,
            ws.data_ptr(), ws.numel(), _lib.stream()))
        torch.cuda.synchronize()
    finally:
        restore_hooks()
    third = torch.tensor(1., dtype=torch.float32) / torch.tensor(
        3., dtype=torch.float32)
    want = (case['total'] * third.double()).float().double()
    assert_equal(from_cl(out, c), want, (nseg, case['mode'], niter))
