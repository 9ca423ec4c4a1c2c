"""The Vocos kernels against a float64 oracle with `torch.equal`.

vocos_block_kernel (through pm_convnext_block_cl) in f16 and bf16 on the
inputs of vocos_exact_oracle.py, which make the depthwise conv, the LayerNorm,
the GELU, both contractions and the epilogue exact or - xn on edge rows, h
everywhere - a rounding of an exactly known value that is provably no tie:
every row is compared, edge rows included, with no tolerance. A rounding toward
zero of xn or h, a bias added on the wrong side of a rounding, a wrong tap,
halo, hidden chunk, tile row or column moves outputs by whole units.

fp32 is not bit-exact (the last ulp of the device's rstd reaches the output):
it is held per element to the bound the oracle derives from a relative error
of 2**-22 in rstd and one fp32 rounding per operation on edge rows. No
tolerance here was taken from the code under test.

vocos_gemm_kernel (conv_pre, embed, head.out) through its own entry
pm_vocos_gemm_cl: integer inputs, all three modes exact, both input layouts,
both gbias forms, the two live columns of the ninth column block at N = 1026,
rows short of, at and past a 32-row wave tile and a 64-row workgroup tile.

The case tables are checked without a GPU by test_cpu_vocos_exact.py, which
also shows that the comparison rejects planted defects. What these inputs
cannot see (the shape of GELU, LayerNorm on generic rows) stays with
test_gpu_vocos.py.
"""
import pytest
import torch

import exact_oracle as E
import vocos_exact_oracle as V

pytestmark = pytest.mark.gpu

LEAVES = ('dwconv.weight', 'dwconv.bias', 'norm.weight', 'norm.bias',
          'pwconv1.weight', 'pwconv1.bias', 'pwconv2.weight', 'pwconv2.bias',
          'gamma')


def lib():
    from promonet_amd import _lib
    return _lib


def run_block(device, mode, x, p):
    _lib = lib()
    batch, frames, channels = x.shape
    hidden = p['pwconv1.weight'].shape[0]
    tensors = [p[k].float().contiguous().to(device) for k in LEAVES]
    x = x.contiguous().to(device)
    y = torch.full_like(x, float('nan'))
    code = _lib.DTYPES[mode]
    ws = torch.empty(_lib.lib().pm_convnext_block_workspace_bytes(
        code, channels, hidden), dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().pm_convnext_block_cl(
        code, _lib.ptr(x), _lib.ptr(y), *[_lib.ptr(t) for t in tensors],
        batch, frames, channels, hidden, ws.data_ptr(), ws.numel(),
        _lib.stream()))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize('mode', ['f16', 'bf16'])
@pytest.mark.parametrize('hidden', V.BLOCK_HIDDEN)
@pytest.mark.parametrize('batch,frames', V.BLOCK_SHAPES)
def test_block_exact(device, mode, hidden, batch, frames):
    case = V.block_case(mode, hidden, batch, frames)
    assert case['bits'] <= E.EXACT_BITS and case['margin'] >= V.TIE_MARGIN
    got = run_block(device, mode, case['x'], case['p']).double()
    want = case['want']
    assert torch.equal(want.float().double(), want)
    # (batch, frame, channel: first_difference's batch, column, channel)
    assert torch.equal(got, want), E.first_difference(
        got.transpose(1, 2), want.transpose(1, 2))
    again = run_block(device, mode, case['x'], case['p']).double()
    assert torch.equal(again, got), 'two runs differ'


@pytest.mark.parametrize('hidden', V.BLOCK_HIDDEN)
@pytest.mark.parametrize('batch,frames', V.BLOCK_SHAPES)
def test_block_fp32_within_the_derived_bound(device, hidden, batch, frames):
    case = V.block_case('fp32', hidden, batch, frames)
    got = run_block(device, 'fp32', case['x'], case['p'])
    assert torch.isfinite(got).all()
    error = (got.double() - case['want']).abs()
    ratio = error / case['bound']
    print(f'fp32 H {hidden} ({batch}, {frames}): max error {error.max():.3e}, '
          f'largest error / bound {ratio.max():.3f}, {int((error > 0).sum())} '
          f'of {error.numel()} elements differ')
    worst = ratio.argmax().item()
    assert (error <= case['bound']).all(), (
        worst, error.flatten()[worst].item(),
        case['bound'].flatten()[worst].item())
    again = run_block(device, 'fp32', case['x'], case['p'])
    assert torch.equal(again, got), 'two runs differ'


def run_gemm(device, mode, case):
    _lib = lib()
    x, w = case['x'], case['w']
    n, k, taps = w.shape
    batch = x.shape[0]
    frames = x.shape[2] if case['cf'] else x.shape[1]
    gbias = case['gbias']
    tensors = [t.contiguous().to(device) for t in (x, w, case['bias'])]
    g = None if gbias is None else gbias.contiguous().to(device)
    out = torch.full((batch, frames, n), float('nan'), device=device)
    code = _lib.DTYPES[mode]
    ws = torch.empty(_lib.lib().pm_vocos_gemm_workspace_bytes(
        code, taps, k, n), dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().pm_vocos_gemm_cl(
        code, taps, int(case['cf']), *[_lib.ptr(t) for t in tensors],
        None if g is None else _lib.ptr(g), 0 if g is None else g.shape[0],
        _lib.ptr(out), batch, frames, k, n, ws.data_ptr(), ws.numel(),
        _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('mode', V.MODES)
@pytest.mark.parametrize('name,gbatch', V.gemm_table())
@pytest.mark.parametrize('batch,frames', V.GEMM_SHAPES)
def test_gemm_exact(device, mode, name, gbatch, batch, frames):
    case = V.gemm_case(mode, name, gbatch, batch, frames)
    assert case['bits'] <= E.EXACT_BITS
    got = run_gemm(device, mode, case).double()
    want = case['want']
    assert torch.equal(got, want), E.first_difference(
        got.transpose(1, 2), want.transpose(1, 2))


def test_gemm_entry_rejects_bad_arguments(device):
    _lib = lib()
    case = V.gemm_case('fp32', 'embed', 0, 1, 1)
    x, w, bias = [t.to(device) for t in (case['x'], case['w'], case['bias'])]
    out = torch.zeros(1, 1, 512, device=device)
    ws = torch.empty(_lib.lib().pm_vocos_gemm_workspace_bytes(0, 7, 512, 512),
                     dtype=torch.uint8, device=device)

    def call(taps=7, cf=0, k=512, gbias=None, gbatch=0, size=ws.numel()):
        return _lib.lib().pm_vocos_gemm_cl(
            0, taps, cf, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), gbias,
            gbatch, _lib.ptr(out), 1, 1, k, 512, ws.data_ptr(), size,
            _lib.stream())

    assert call() == 0
    for bad in (dict(taps=3), dict(taps=1, cf=1), dict(k=504), dict(k=0),
                dict(gbias=_lib.ptr(bias), gbatch=2), dict(size=ws.numel() - 1)):
        assert call(**bad) != 0, bad
    assert _lib.lib().pm_vocos_gemm_workspace_bytes(0, 3, 512, 512) == 0
