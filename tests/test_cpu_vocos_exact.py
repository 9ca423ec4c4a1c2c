"""The Vocos exact tests' oracle and case table (vocos_exact_oracle.py),
checked without a GPU.

  preconditions   every case of the table stays inside the exact domain: the
                  contractions and the epilogue within EXACT_BITS, every xn
                  at least TIE_MARGIN from a rounding tie, every
                  pre-activation beyond +-16, the f16 operands below 65504 -
                  and the cases do hold values the 16-bit types cannot (a
                  rounding is exercised, ties to even among them).
  oracle          on these inputs it equals vocos_oracle.convnext_block run in
                  float64 (fp32 mode: no rounding of xn or h to compare).
  emulation       vocos_block_kernel restated step by step in fp32 gives the
                  oracle's bits in f16 and bf16.
  planted defects the comparison of the GPU test rejects each of them, applied
                  to that emulation: `torch.equal` for the 16-bit modes and
                  for the contraction kernel.

What the construction cannot see: the shape of GELU (a tanh approximation is
identical where |v| >= 16, which is every pre-activation here) and LayerNorm
on generic rows, whose mean and variance are not exact. Both stay with the
fp32 gate of test_gpu_vocos.py.
"""
import pytest
import torch

import exact_oracle as E
import vocos_exact_oracle as V
import vocos_oracle

HALF_MODES = ('f16', 'bf16')


# ---------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', HALF_MODES)
@pytest.mark.parametrize('hidden', V.BLOCK_HIDDEN)
def test_block_cases_are_inside_the_exact_domain(mode, hidden):
    for batch, frames in V.BLOCK_SHAPES:
        case = V.block_case(mode, hidden, batch, frames)    # raises NotExact
        assert 0 < case['bits'] <= E.EXACT_BITS
        assert case['margin'] >= V.TIE_MARGIN
        assert case['v1'].abs().min() >= 16
        if mode == 'f16':
            for t in (case['xn'], case['v1'], case['h']):
                assert t.abs().max() < E.F16_MAX
        want = case['want']
        assert torch.equal(want.float().double(), want)


def test_the_construction_is_what_the_docstring_says():
    p, tau, sign = V.block_weights(192, 192)
    assert sum(V.TAP_CLASSES) == V.CHANNELS
    assert all(n % 2 == 0 for n in V.TAP_CLASSES)
    assert torch.equal(torch.bincount(tau), torch.tensor(V.TAP_CLASSES))
    # one tap of +-1 a channel
    dw = p['dwconv.weight']
    assert torch.equal(dw.abs().sum((1, 2)), torch.ones(V.CHANNELS))
    # g odd, beta even: +-g + beta is never 0 and, beyond the type's
    # integers, never a tie
    assert (p['norm.weight'] % 2 == 1).all() and (p['norm.bias'] % 2 == 0).all()
    assert torch.log2(p['gamma']).frac().eq(0).all()
    x = V.block_input(3, 9, tau, sign, 1)
    s = x / (8 * sign)
    assert torch.equal(s.abs(), torch.ones_like(s))
    for tap in range(7):
        assert not s[:, :, tau == tap].sum(-1).any()
    # every channel feeds a hidden unit and every hidden unit an output
    for hidden in V.BLOCK_HIDDEN:
        p, _, _ = V.block_weights(hidden, hidden)
        assert p['pwconv2.weight'].abs().sum(0).min() > 0
        assert p['pwconv1.weight'].abs().sum(0).min() > 0


@pytest.mark.parametrize('mode', HALF_MODES)
def test_interior_rows_are_integers_and_roundings_are_exercised(mode):
    case = V.block_case(mode, 192, 3, 130)
    xn, v1, h = case['xn'][:, 3:-3], case['v1'][:, 3:-3], case['h'][:, 3:-3]
    assert torch.equal(xn, xn.round()) and xn.abs().min() >= 1
    assert torch.equal(v1, v1.round())
    # values the type cannot hold: h = cvt(v1) rounds, at ties too
    moved = h != v1.clamp(min=0)
    assert moved.any()
    grid = 2. if mode == 'f16' else 16.
    ties = (v1 > V.BIG_B1) & (v1 % grid == grid / 2)
    assert ties.any() and (h[ties] % (2 * grid) == 0).all()
    if mode == 'bf16':
        big = case['p']['norm.weight'].abs() == V.BIG_G
        assert big.sum() == 4
        assert (xn[:, :, big] % 4 == 0).all() and (xn[:, :, big].abs() > 500).all()
    # edge rows: xn is a genuine rounding
    edge = case['xn'][:, :3]
    assert not torch.equal(edge, edge.round())


def test_tie_margin_and_truncation_by_hand():
    # f16 grid in [1, 2) is 2**-10, bf16's 2**-7
    v = torch.tensor([1. + 2. ** -11 + 2. ** -20], dtype=torch.float64)
    assert abs(V.tie_margin(v, 'f16') * v.item() - 2. ** -20) < 1e-15
    assert abs(V.tie_margin(torch.tensor([1.25], dtype=torch.float64), 'bf16')
               - 2. ** -8 / 1.25) < 1e-15
    # just below a power of two the grid halves
    v = torch.tensor([1. - 2. ** -13], dtype=torch.float64)
    assert abs(V.tie_margin(v, 'f16') * v.item() - 2. ** -13) < 1e-15
    v = torch.tensor([2049., -2051., 2050., .1], dtype=torch.float32)
    assert V.cvt(v, 'f16').tolist()[:3] == [2048., -2052., 2050.]
    assert V.cvt(v, 'f16', truncate=True).tolist()[:3] == [2048., -2050., 2050.]
    assert abs(V.cvt(v, 'f16', truncate=True)[3].item()) < .1
    v = torch.tensor([515., -517., 257.], dtype=torch.float32)
    assert V.cvt(v, 'bf16').tolist() == [516., -516., 256.]
    assert V.cvt(v, 'bf16', truncate=True).tolist() == [512., -516., 256.]


def test_preconditions_are_enforced():
    case = V.block_case('bf16', 64, 1, 5)
    x, p = case['x'], dict(case['p'])
    broken = dict(p)
    broken['pwconv1.bias'] = p['pwconv1.bias'] * 0 + 1
    with pytest.raises(V.NotExact, match='pre-activation'):
        V.block(x, broken, 'bf16')
    broken = dict(p)
    broken['norm.weight'] = p['norm.weight'] * .001
    with pytest.raises(V.NotExact):
        V.block(x, broken, 'bf16')
    unbalanced = x.clone()
    unbalanced[0, 2, 7] *= -1
    with pytest.raises(V.NotExact, match='balanced'):
        V.block(unbalanced, p, 'bf16')
    wide = V.gemm_case('f16', 'embed', 0, 1, 1)
    x = wide['x'].clone()
    x[0, 0, 0] = 70000.
    with pytest.raises(V.NotExact, match='f16 range'):
        V.gemm(x, wide['w'], wide['bias'], None, 'f16', False)


@pytest.mark.parametrize('mode', V.MODES)
def test_gemm_cases_are_exact(mode):
    for name, gbatch in V.gemm_table():
        for batch, frames in V.GEMM_SHAPES:
            case = V.gemm_case(mode, name, gbatch, batch, frames)
            assert 0 < case['bits'] <= E.EXACT_BITS
            assert case['want'].shape == (batch, frames,
                                          V.GEMM_KERNELS[name][3])
    assert sorted(b * t for b, t in V.GEMM_SHAPES) == [1, 31, 33, 100, 130]
    # the roundings of the large operands are exercised
    x = V.gemm_case('bf16', 'head', 0, 2, 65)['x']
    assert not torch.equal(V.cvt(x, 'bf16'), x.double())
    assert not torch.equal(V.cvt(x, 'f16'), x.double())


# ---------------------------------------------------------------------------
# the oracle against the restatement the project already trusts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('batch,frames', V.BLOCK_SHAPES)
def test_oracle_equals_the_restatement_in_float64(batch, frames):
    case = V.block_case('fp32', 192, batch, frames)
    state = {'b.' + k: v.double() for k, v in case['p'].items()}
    want = vocos_oracle.convnext_block(
        case['x'].double().transpose(1, 2), state, 'b.').transpose(1, 2)
    # the only difference: eps is added in fp32 by the kernel and the oracle
    # (64 + 1e-6f is 64), in float64 by layer_norm: 1e-6 / 64 / 2 = 7.8e-9
    # relative in rstd, and so in every term of the output
    scale = case['want'].abs().max().item()
    assert (case['want'] - want).abs().max().item() <= 1e-7 * scale
    assert (case['bound'] > 0).all()


def test_gemm_oracle_equals_conv1d_and_linear():
    case = V.gemm_case('fp32', 'conv_pre', 'B', 3, 11)
    want = torch.nn.functional.conv1d(
        case['x'].double(), case['w'].double(), case['bias'].double(),
        padding=3) + case['gbias'].double()[:, :, None]
    assert torch.equal(case['want'], want.transpose(1, 2))
    case = V.gemm_case('fp32', 'head', 0, 3, 11)
    want = torch.nn.functional.linear(
        case['x'].double(), case['w'].double()[:, :, 0], case['bias'].double())
    assert torch.equal(case['want'], want)
    # channels-last k7: utterances do not leak into each other
    case = V.gemm_case('fp32', 'embed', 0, 3, 11)
    alone, _ = V.gemm(case['x'][1:2], case['w'], case['bias'], None, 'fp32',
                      False)
    assert torch.equal(case['want'][1:2], alone)


# ---------------------------------------------------------------------------
# the emulation and the planted defects
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', HALF_MODES)
@pytest.mark.parametrize('hidden', V.BLOCK_HIDDEN)
def test_fp32_emulation_gives_the_oracles_bits(mode, hidden):
    for batch, frames in V.BLOCK_SHAPES:
        case = V.block_case(mode, hidden, batch, frames)
        got = V.emulate_block(case['x'], case['p'], mode).double()
        assert torch.equal(got, case['want']), (batch, frames)


def test_fp32_emulation_is_within_the_derived_bound():
    for batch, frames in V.BLOCK_SHAPES:
        case = V.block_case('fp32', 192, batch, frames)
        got = V.emulate_block(case['x'], case['p'], 'fp32').double()
        assert ((got - case['want']).abs() <= case['bound']).all()


BLOCK_DEFECTS = ('truncate xn', 'truncate h', 'b1 after rounding',
                 'tap off by one', 'halo across utterances', 'chunk skipped',
                 'chunk without hc', 'gamma before b2')


@pytest.mark.parametrize('mode', HALF_MODES)
@pytest.mark.parametrize('defect', BLOCK_DEFECTS)
def test_planted_block_defect_is_rejected(mode, defect):
    # (4, 6): edge rows only; (19, 7): one interior row an utterance
    for batch, frames in ((4, 6), (19, 7)):
        case = V.block_case(mode, 192, batch, frames)
        got = V.emulate_block(case['x'], case['p'], mode, defect).double()
        differ = int((got != case['want']).sum())
        print(f'{mode} {defect} ({batch}, {frames}): {differ} of '
              f'{got.numel()} elements differ')
        assert not torch.equal(got, case['want']), (batch, frames)


@pytest.mark.parametrize('defect', ('truncate xn', 'truncate h'))
def test_rounding_mode_shows_on_interior_rows_too(defect):
    """f16 holds every interior xn, so a truncated xn shows there in bf16
    only; a truncated h shows in both types (pre-activations beyond 2048)."""
    for mode in HALF_MODES:
        case = V.block_case(mode, 192, 3, 130)
        got = V.emulate_block(case['x'], case['p'], mode, defect).double()
        interior = (got != case['want'])[:, 3:-3].any().item()
        assert interior == (defect == 'truncate h' or mode == 'bf16'), mode


@pytest.mark.parametrize('mode', V.MODES)
def test_planted_gemm_defect_is_rejected(mode):
    case = V.gemm_case(mode, 'head', 0, 3, 11)
    args = (case['x'], case['w'], case['bias'], None, mode, False)
    assert torch.equal(V.emulate_gemm(*args).double(), case['want'])
    got = V.emulate_gemm(*args, defect='last column block dropped').double()
    assert torch.equal(got[:, :, :1024], case['want'][:, :, :1024])
    assert (got[:, :, 1024:] != case['want'][:, :, 1024:]).any()
    case = V.gemm_case(mode, 'conv_pre', 'B', 3, 11)
    got = V.emulate_gemm(case['x'], case['w'], case['bias'], case['gbias'],
                         mode, True, defect='gbias of the wrong utterance')
    assert not torch.equal(got.double(), case['want'])


def test_gemm_entry_checks_its_arguments():
    """pm_vocos_gemm_cl refuses on the host, before any launch (the pointers
    here are never followed)."""
    import ctypes
    from promonet_amd import _lib
    library = _lib.lib()
    fake = ctypes.addressof(ctypes.create_string_buffer(64))
    size = library.pm_vocos_gemm_workspace_bytes(_lib.PM_F16, 7, 512, 1026)
    assert size == 1152 * 7 * 512 * 2       # N padded to the 128-column block
    assert library.pm_vocos_gemm_workspace_bytes(_lib.PM_F32, 1, 80, 512) == \
        512 * 80 * 4

    def call(dtype=_lib.PM_F16, taps=7, cf=0, x=fake, gbias=None, gbatch=0,
             batch=2, frames=5, k=512, n=1026, ws=fake, bytes_=size):
        return library.pm_vocos_gemm_cl(
            dtype, taps, cf, x, fake, fake, gbias, gbatch, fake, batch,
            frames, k, n, ws, bytes_, None)

    for bad in (dict(dtype=7), dict(taps=3), dict(taps=1, cf=1), dict(x=None),
                dict(batch=0), dict(frames=0), dict(k=0), dict(k=8),
                dict(k=504), dict(n=0), dict(gbias=fake, gbatch=3)):
        assert call(**bad) == _lib.PM_EINVAL, bad
    for bad in (dict(ws=None), dict(bytes_=size - 1)):
        assert call(**bad) == _lib.PM_ENOMEM, bad
    for name in ('dtype', 'taps', 'in_channels', 'out_channels'):
        args = dict(dtype=_lib.PM_F16, taps=7, in_channels=512,
                    out_channels=512)
        args[name] = 9 if name == 'dtype' else 0
        assert library.pm_vocos_gemm_workspace_bytes(*args.values()) == 0
