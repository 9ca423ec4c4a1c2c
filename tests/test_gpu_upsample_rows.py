"""The upsamplers' output stores, exactly: `torch.equal` with
`F.conv_transpose1d`, no tolerance.

With 16-bit operands every wave turns its 32-column tiles round in LDS and
stores runs of whole rows (pm_store_rows, pm_conv.h): the wide (r = 8)
upsampler 32 columns at a time at C_in = 256 and 8 at C_in = 512
(conv_upsample_kernel), the r = 2 upsamplers 32 (conv_single_kernel). With a
forced group count (`pm_debug_force`) the wide upsampler stores straight from
the MFMA layout. A store that lands in the wrong row, column or channel, that
is dropped or that goes past an utterance's end shows here as whole units of
the value grid: the inputs are exact_oracle.py's small integers, every sum is
exact in fp32 and independent of its order.

Lengths: below one 32-column wave tile (1, 31), exactly one wave's two tiles
and one column over (64, 65), one and two 128-column workgroup tiles plus one
column (129, 257). The ragged case ends the second utterance two columns into
its second tile.
"""
import pytest
import torch

import exact_oracle as E
from util import from_cl, to_cl

pytestmark = pytest.mark.gpu

SHAPES = ((256, 128, 8), (512, 256, 8), (128, 64, 2), (64, 32, 2))
LENGTHS = (1, 31, 64, 65, 129, 257)
RAGGED = (257, 130)
MODES = ('bf16', 'f16')
SENTINEL = -12345.


def lib():
    from promonet_amd import _lib
    return _lib


def force_groups(groups):
    _lib = lib()
    _lib.check(_lib.lib().pm_debug_force(0, groups))


def workspace(device, c_in, c_out, rate):
    size = lib().lib().pm_op_workspace_bytes(c_in, c_out, 2 * rate)
    return torch.empty(size, dtype=torch.uint8, device=device)


def run(device, mode, x_cl, w, bias, c_in, c_out, rate, ws, lengths=None):
    """`out` starts as SENTINEL everywhere"""
    _lib = lib()
    batch, length, _ = x_cl.shape
    out = torch.full((batch, length * rate, c_out), SENTINEL, device=device)
    if lengths is None:
        _lib.check(_lib.lib().pm_conv_transpose_cl(
            _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out), _lib.ptr(w),
            _lib.ptr(bias), batch, length, c_in, c_out, rate, 1,
            ws.data_ptr(), ws.numel(), _lib.stream()))
    else:
        _lib.check(_lib.lib().pm_conv_transpose_ragged_cl(
            _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out), _lib.ptr(w),
            _lib.ptr(bias), lengths.data_ptr(), batch, length, c_in, c_out,
            rate, 1, ws.data_ptr(), ws.numel(), _lib.stream()))
    torch.cuda.synchronize()
    return out


def assert_equal(got, want, detail):
    got = got.double().cpu()
    assert torch.equal(got, want), (detail, E.first_difference(got, want))


@pytest.mark.parametrize('groups', (0, 2))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('c_in,c_out,rate', SHAPES)
def test_dense(device, mode, c_in, c_out, rate, groups):
    ws = workspace(device, c_in, c_out, rate)
    try:
        force_groups(groups)
        for length in LENGTHS:
            case = E.upsample_case(mode, c_in, c_out, rate, length)
            assert case['bits'] <= E.EXACT_BITS, case['bits']
            out = run(device, mode, to_cl(case['x']).to(device),
                      case['w'].to(device), case['bias'].to(device), c_in,
                      c_out, rate, ws)
            assert_equal(from_cl(out, c_out), case['want'], length)
    finally:
        force_groups(0)


@pytest.mark.parametrize('groups', (0, 2))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('c_in,c_out,rate', SHAPES)
def test_ragged(device, mode, c_in, c_out, rate, groups):
    """Each utterance equals itself alone (the rows of x past its length read
    as zero), and nothing is written past its end"""
    ws = workspace(device, c_in, c_out, rate)
    length = max(RAGGED)
    case = E.upsample_case(mode, c_in, c_out, rate, length)
    assert case['bits'] <= E.EXACT_BITS, case['bits']
    lengths = torch.tensor(RAGGED, dtype=torch.int32, device=device)
    try:
        force_groups(groups)
        out = run(device, mode, to_cl(case['x']).to(device),
                  case['w'].to(device), case['bias'].to(device), c_in, c_out,
                  rate, ws, lengths)
    finally:
        force_groups(0)
    got = from_cl(out, c_out)
    for b, valid in enumerate(RAGGED):
        want, bits = E.conv_transpose(
            case['x'][b:b + 1, :, :valid], case['w'], case['bias'], mode, rate)
        assert bits <= E.EXACT_BITS
        assert_equal(got[b:b + 1, :, :valid * rate], want, (b, valid))
        assert (out[b, valid * rate:] == SENTINEL).all(), (b, valid)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('c_in,c_out,rate', SHAPES[:2])
def test_row_stores_match_direct_stores(device, mode, c_in, c_out, rate):
    """Random (non-integer) inputs: the planner's kernel against the direct
    stores of the forced group counts, bit for bit, ragged batch included"""
    ws = workspace(device, c_in, c_out, rate)
    gen = torch.Generator().manual_seed(c_in)
    w = (.05 * torch.randn(c_in, c_out, 2 * rate, generator=gen)).to(device)
    bias = torch.randn(c_out, generator=gen).to(device)
    ragged = torch.tensor(RAGGED, dtype=torch.int32, device=device)
    try:
        for length in LENGTHS:
            x_cl = torch.randn(2, length, c_in, generator=gen).to(device)
            for lengths in ((None, ragged) if length == max(RAGGED)
                            else (None,)):
                outs = []
                for groups in (0, 1, 2):
                    force_groups(groups)
                    outs.append(run(device, mode, x_cl, w, bias, c_in, c_out,
                                    rate, ws, lengths))
                assert outs[0].isfinite().all()
                for groups, out in zip((1, 2), outs[1:]):
                    assert torch.equal(outs[0], out), (
                        length, groups, lengths is not None)
    finally:
        force_groups(0)
