"""The exact tests' oracle and case table (exact_oracle.py), checked without a
GPU: every case of the table is inside the exactness bound and the f16 range,
the sparse cases cover every weight position, the oracle agrees with the
restatement the project already trusts, `round_operand` gives bit patterns
written out by hand - and the comparison has teeth: the oracle with ONE defect
planted stands in for a wrong kernel, and `torch.equal` rejects each.

Why the exact tests exist is the number test_planted_indexing_defect prints:
on the random-normal inputs of test_gpu_kernels.py (C 128, k 11, d 3), by
util.rel_err, one tap dropped at one column measures 1.1e-3 and one column
read from its neighbour 5.9e-3 - both one product of every output of that
column, both under the bf16 gate TOL_BLOCK = 1e-2 (asserted). The other two
turned out to EXCEED that gate and are left as they are: two input channels
swapped in one row (its k = 11 taps: 22 products) measures 1.13e-2, just over;
dilation 3 taken as 2 for one tap (C products of every output) 1.7e-1 - the
tolerance tests see those two. On the exact inputs each of the four moves
outputs by thousands of whole units of q.

Three iterations (the lifted cases of exact_oracle.py): every case is built
and its conditions written out once more (lifted_conditions), the bits and the
largest operand printed; the planted defects of three iterations - dilations
swapped, the third iteration dropped, truncation, a hidden LeakyReLU left
out, one tile with the halo of two iterations - are held by the SHARE of the
elements they move."""
import pytest
import torch
import torch.nn.functional as F

import exact_oracle as E
import restatement
from util import rel_err

TOL_BLOCK_BF16 = 1e-2       # test_gpu_kernels.py


# ---------------------------------------------------------------------------
# The case table
# ---------------------------------------------------------------------------
def f16_range(mode, *operands):
    """f16 cases stay under 65504 in every operand (16-bit f16 modes)."""
    if mode in ('f16', 'f16x3', 'f16a2'):
        for t in operands:
            assert t.abs().max().item() < E.F16_MAX


@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('channels', E.ITERATION_CHANNELS)
def test_iteration_cases_exact(mode, channels):
    for k in E.ITERATION_KERNELS:
        for d, length, store_mode in E.ITERATION_RUNS:
            case = E.iteration_case(mode, channels, k, d, length, store_mode)
            assert case['bits'] <= E.EXACT_BITS
            f16_range(mode, *case['operands'], *case['w'])
            # every operand of the dense construction is an integer
            for t in case['operands']:
                assert torch.equal(t, t.round())


@pytest.mark.parametrize('mode', ['f16', 'bf16'])
def test_wide_iteration_cases_exact(mode):
    for c, k, length in E.ITERATION_WIDE:
        case = E.iteration_wide_case(mode, c)
        assert case['bits'] <= E.EXACT_BITS
        f16_range(mode, *case['operands'])
        # batch 2: >= 150 wide tiles, the last one ragged
        tile = (256 if c == 128 else 192) - (k - 1)
        assert -(-length // tile) * E.BATCH >= 150 and length % tile


def block_operands(case, mode):
    """fp32 activations in front of every conv of a Block case."""
    out = []
    y = case['x'].double()
    w1, b1, w2, b2 = case['w']
    for n, d in enumerate(case['dilations']):
        a1 = E.lrelu32(y.float())
        h, _ = E.conv(a1, w1[n], E.round_operand(b1[n], mode, 'bias'), mode, d)
        out += [a1, E.lrelu32(h.float())]
        y, _ = E.block_iteration(y.float(), w1[n], b1[n], w2[n], b2[n], mode, d)
    return out


def lifted_conditions(x, w, mode, dilations, signed):
    """The conditions of a three-iteration Block, written out on the values
    in front of its six convs (E.assert_lifted holds the same at build time);
    returns the largest operand."""
    w1, b1, w2, b2 = w
    before = E.lifted_operands(x, w, mode, dilations)
    operands = [E.lrelu32(t) for t in before]
    # under 65504 in EVERY mode: the clamp is not what makes a case pass
    largest = max(t.abs().max().item() for t in operands)
    assert largest < E.F16_MAX
    for t in operands:      # integers: v * 0.1f met multiples of 10 only
        assert torch.equal(t, t.round())
    for n in range(3):
        trunk, hidden = before[2 * n], before[2 * n + 1]
        assert (trunk < 0).float().mean() >= .25, n
        assert torch.equal(trunk, (trunk / 10).round() * 10)
        last = n == 2
        if n == signed:
            assert (hidden < 0).float().mean() >= .25
            assert torch.equal(hidden, (hidden / 10).round() * 10)
            assert (w1[n] != 0).sum(dim=(1, 2)).eq(1).all()
            assert set(w1[n].unique().tolist()) == {-10., 0., 10.}
            assert set(b1[n].unique().tolist()) <= {-10., 0., 10.}
        else:
            assert (hidden >= 0).all()      # its LeakyReLU is the identity
            assert set(w1[n].unique().tolist()) == {0., 1.}
            assert (w1[n] != 0).sum(dim=(1, 2)).le(2).all()
            lift = b1[n]
            assert (lift == lift[0]).all() and lift[0] > 0
            for half in ('f16', 'bf16'):    # 16 bits hold it
                assert torch.equal(
                    E.round_operand(lift, half, 'bias'), lift.double())
            # no smaller than weights per row x the largest negative operand
            per_row = (w1[n] != 0).sum(dim=(1, 2)).max().item()
            assert lift[0] >= per_row * -operands[2 * n].min().item()
        unit = 1. if last else 10.
        assert set(w2[n].unique().tolist()) == {-unit, 0., unit}
        assert (w2[n] != 0).sum(dim=(1, 2)).le(2).all()
        assert b2[n].abs().max() <= (9. if last else 10.)
        assert torch.equal(b2[n], (b2[n] / unit).round() * unit)
        for weight in (w1[n], w2[n]):
            hit = weight != 0
            assert hit.any(dim=(0, 2)).all()        # every input channel
            assert hit.any(dim=(0, 1)).all()        # every tap
    return largest


@pytest.mark.parametrize('niter', [1, 2, 3])
@pytest.mark.parametrize('channels,kernel_size', E.BLOCK_SHAPES)
def test_block_cases_exact(channels, kernel_size, niter):
    for mode in E.block_modes(channels):
        assert E.block_requests(mode, channels, kernel_size)
        for run in range(3):
            case = E.block_case(mode, channels, kernel_size, niter, run)
            assert case['bits'] <= E.EXACT_BITS
            if niter < 3:
                f16_range(mode, *block_operands(case, mode))
                continue
            # the signed iteration rotates over the runs; the lengths are the
            # runs' of three iterations
            assert case['signed'] == run
            assert sorted(case['dilations']) == [1, 3, 5]
            largest = lifted_conditions(
                case['x'], case['w'], mode, case['dilations'], run)
            assert largest == case['largest'] <= max(case['worst']) * (
                1 + 2. ** -8)
            print(f'{mode} C {channels} k {kernel_size} run {run}: '
                  f'{case["bits"]:.1f} bits, largest operand {largest:g}')
    if niter == 3:
        columns = E.block_geometry('bf16', channels, kernel_size)[1]
        runs = E.block_runs('bf16', channels, kernel_size, 3)
        assert [(r[0], r[1], r[3]) for r in runs] == [
            (2, 9 * columns + 37, 0), (3, 2 * columns + 1, 2), (2, 61, 1)]
    # the kernels that exist in one form only are in the table in that form
    forms = {(c, k): [E.block_form('bf16', c, k, r)
                      for r in E.block_requests('bf16', c, k)]
             for c, k in E.BLOCK_SHAPES}
    assert forms[128, 7] == ['walked', 'skewed'] and forms[256, 3] == [
        'walked', 'skewed']
    assert forms[128, 11] == ['skewed'] and forms[256, 7] == ['skewed']


@pytest.mark.parametrize('channels,kernel_size', E.BLOCK_SHAPES)
def test_sparse_cases_cover_every_weight_position(channels, kernel_size):
    """2 (c): over the niter = 2 cases of a shape, every (c_in, tap) position
    of every weight matrix (iteration x conv1 / conv2) is non-zero at least
    once."""
    seen = None
    for mode in E.block_modes(channels):
        for run in range(3):
            w = E.block_case(mode, channels, kernel_size, 2, run)['w']
            for weight in w[0] + w[2]:
                assert (weight != 0).sum(dim=(1, 2)).eq(2).all()
                assert set(weight.unique().tolist()) == {-10., 0., 10.}
            hit = torch.stack([(m != 0).any(dim=0) for m in w[0] + w[2]])
            seen = hit if seen is None else seen | hit
    assert seen.shape == (4, channels, kernel_size) and seen.all()


@pytest.mark.parametrize('mode', E.MODES)
def test_other_cases_exact(mode):
    for c in E.MRF_CHANNELS:
        for niter in (1, 2, 3):
            for run in range(len(E.MRF_LENGTHS)):
                case = E.mrf_case(mode, c, niter, run)
                assert case['bits'] <= E.EXACT_BITS
                if niter < 3:
                    continue
                # three lifted Blocks on one input, their sum exact in fp32
                largest = max(
                    lifted_conditions(case['x'], w, mode, case['dilations'],
                                      case['signed'])
                    for w in case['blocks'])
                assert largest == case['largest']
                total = case['total']
                assert torch.equal(total.float().double(), total)
                print(f'MRF {mode} C {c} L {case["length"]}: '
                      f'{case["bits"]:.1f} bits, largest operand {largest:g}, '
                      f'largest sum {total.abs().max().item():g}')
        columns = 768 if mode in ('f16', 'bf16') else 512
        assert E.mrf_lengths(mode, 3) == (
            1, 61, 2 * columns + 1, 5 * columns + 37)
        assert E.mrf_lengths(mode, 2) == E.MRF_LENGTHS
    for shape in E.UPSAMPLE_SHAPES:
        for length in E.UPSAMPLE_LENGTHS:
            case = E.upsample_case(mode, *shape, length)
            assert case['bits'] <= E.EXACT_BITS
            f16_range(mode, case['x'], case['w'])
    if mode in ('f16', 'bf16'):
        for _, length, drawn in E.UPSAMPLE_LONG:
            case = E.upsample_long_case(mode, length, drawn)
            assert case['bits'] <= E.EXACT_BITS
            f16_range(mode, case['x'], case['w'])
    if mode in E.INPUT_MODES:
        for shape in E.INPUT_SHAPES:
            for run in range(len(E.INPUT_RUNS)):
                case = E.input_case(mode, *shape, run)
                assert case['bits'] <= E.EXACT_BITS
                f16_range(mode, case['x'], case['w'])
    if mode in ('f16', 'f16x3', 'f16a2'):
        case = E.f16_edge_case(mode)
        assert case['bits'] <= E.EXACT_BITS
        # the one case built to cross 65504, in both convs
        a1 = E.lrelu32(case['x'])
        assert a1.max() > E.F16_MAX
        h, _ = E.conv(a1, case['w'][0],
                      E.round_operand(case['w'][1], mode, 'bias'), mode, 3)
        assert h.max() > E.F16_MAX and torch.isfinite(case['want']).all()


def test_not_exact_is_an_error():
    """Three sparse iterations pass the bound (24.8 - 25.1 bits in bf16, in
    f16 the operands leave the range): the oracle refuses, it never compares
    loosely. So does one operand off the integer grid."""
    for mode in ('bf16', 'f16', 'fp32'):
        for c, k in ((32, 7), (128, 11)):
            w = E.sparse_block(c, k, 3, 1, 0)
            x = E.sparse_input(2, c, 300, 2)
            E.block(x, *[ws[:2] for ws in w], mode, (1, 3))     # two: exact
            with pytest.raises(E.NotExact):
                E.block(x, *w, mode, (1, 3, 5))
    with pytest.raises(E.NotExact):
        x = torch.full((1, 32, 40), 3.)
        E.conv(x * .1, torch.ones(32, 32, 3), torch.zeros(32).double(),
               'fp32')               # 0.3f: a 24-bit operand


# ---------------------------------------------------------------------------
# The oracle against what the project already trusts
# ---------------------------------------------------------------------------
def state_of(w, prefix='p'):
    state = {}
    for n in range(len(w[0])):
        state[f'{prefix}.convs1.{n}.weight'] = w[0][n]
        state[f'{prefix}.convs1.{n}.bias'] = w[1][n]
        state[f'{prefix}.convs2.{n}.weight'] = w[2][n]
        state[f'{prefix}.convs2.{n}.bias'] = w[3][n]
    return state


@pytest.mark.parametrize('niter', [1, 2, 3])
def test_fp32_oracle_equals_restatement(niter):
    cases = [E.block_case('fp32', 32, 3, niter, 1),
             E.block_case('fp32', 64, 11, niter, 0)]
    if niter == 1:      # padded channels, dense
        cases.append(dict(
            w=tuple([t] for t in E.dense_iteration(48, 7, 5)),
            x=E.dense_input(2, 48, 131, 6), dilations=(3,)))
    for case in cases:
        w, x, dilations = case['w'], case['x'], case['dilations']
        got, _ = E.block(x, *w, 'fp32', dilations)
        want = restatement.block(
            x, state_of(w), 'p', w[0][0].shape[-1], dilations)
        assert want.dtype == torch.float32
        assert torch.equal(got, want.double())
    # the MRF sum: the three Blocks, added
    case = E.mrf_case('fp32', 20, niter, 2)
    want = sum(
        restatement.block(case['x'], state_of(w), 'p', k, case['dilations'])
        for k, w in zip((3, 7, 11), case['blocks']))
    assert torch.equal(case['total'], want.double())
    for shape in ((64, 32, 8), (16, 8, 4)):
        case = E.upsample_case('fp32', *shape, 130)
        want = F.conv_transpose1d(
            F.leaky_relu(case['x'], .1), case['w'], case['bias'],
            stride=shape[2], padding=shape[2] // 2)
        assert torch.equal(case['want'], want.double())
    case = E.input_case('fp32', 40, 32, 6, 1)
    want = F.conv1d(case['x'], case['w'], case['bias'], padding=3) + \
        F.conv1d(case['g'][:, :, None], case['sw'], case['sb'])
    assert torch.equal(case['want'], want.double())


@pytest.mark.parametrize('mode', ['f16', 'bf16', 'f16x3', 'f16a2'])
def test_16bit_oracle_equals_restatement_on_rounded_operands(mode):
    """The un-fused op sequence of restatement.block, fed the operands
    rounded with plain torch casts (written out here, not taken from the
    oracle), in float64."""
    half = torch.bfloat16 if mode == 'bf16' else torch.float16

    def rn(t):
        return t.to(half).float()

    def act(t):
        if mode == 'bf16':
            return rn(t).double()
        if mode == 'f16':
            return rn(t).clamp(max=65504.).double()
        t = t.clamp(-65504., 65504.)
        return rn(t).double() + rn(t - rn(t)).double()

    def weight(t):
        if mode == 'f16x3':
            return rn(t).double() + rn(t - rn(t)).double()
        return rn(t).double()

    def bias(t):
        return rn(t).double() + rn(t - rn(t)).double()

    for c, k, niter, run in ((64, 7, 1, 1), (64, 11, 2, 1), (128, 3, 2, 1),
                             (64, 11, 3, 0), (32, 7, 3, 1), (128, 11, 3, 2)):
        if c > 64 and mode not in ('f16', 'bf16'):
            continue
        case = E.block_case(mode, c, k, niter, run)
        x = case['x'].double()
        w1, b1, w2, b2 = case['w']
        for n, d in enumerate(case['dilations']):
            xt = act(F.leaky_relu(x.float(), .1))
            xt = F.conv1d(xt, weight(w1[n]), bias(b1[n]), dilation=d,
                          padding=restatement.get_padding(k, d))
            xt = act(F.leaky_relu(xt.float(), .1))
            xt = F.conv1d(xt, weight(w2[n]), bias(b2[n]),
                          padding=restatement.get_padding(k, 1))
            x = xt + x
        assert torch.equal(case['raw'], x)
    case = E.upsample_case(mode, 128, 64, 2, 130)
    want = F.conv_transpose1d(
        act(F.leaky_relu(case['x'], .1)), weight(case['w']),
        case['bias'].double(), stride=2, padding=1)
    assert torch.equal(case['want'], want)


# ---------------------------------------------------------------------------
# round_operand against bit patterns written out by hand
# ---------------------------------------------------------------------------
def bits16(v, mode, role='act'):
    hi, lo = E.split_operand(torch.tensor([v], dtype=torch.float32), mode, role)
    half = torch.bfloat16 if mode == 'bf16' else torch.float16
    return tuple(t.to(half).view(torch.int16).item() & 0xffff for t in (hi, lo))


def test_round_operand_bit_patterns():
    # f16: 11 significant bits. 2049 is the tie between 2048 (mantissa even)
    # and 2050, 2051 the one between 2050 and 2052 (even)
    assert bits16(2048., 'f16')[0] == 0x6800
    assert bits16(2049., 'f16')[0] == 0x6800
    assert bits16(2051., 'f16')[0] == 0x6802
    assert bits16(2050.5, 'f16')[0] == 0x6801       # past the tie: 2050
    # bf16: 8 significant bits. 257 is the tie 256 | 258, 259 the tie 258 | 260
    assert bits16(256., 'bf16')[0] == 0x4380
    assert bits16(257., 'bf16')[0] == 0x4380
    assert bits16(259., 'bf16')[0] == 0x4382
    assert bits16(-259., 'bf16')[0] == 0xc382
    assert bits16(257.5, 'bf16')[0] == 0x4381
    # the top of f16: 65504 = 0x7bff; 65520 is the tie to 2**16 = inf, which
    # the activations' min(., 65504) brings back; weights are not clamped
    assert bits16(65504., 'f16')[0] == 0x7bff
    assert bits16(65519., 'f16')[0] == 0x7bff
    assert bits16(65520., 'f16')[0] == 0x7bff
    assert bits16(1e9, 'f16')[0] == 0x7bff
    assert bits16(65520., 'f16', 'weight')[0] == 0x7c00
    assert bits16(-65520., 'f16')[0] == 0xfc00       # no lower clamp (store4)
    assert bits16(65472., 'f16')[0] == 0x7bfe        # 2046 x 32: representable
    assert bits16(65488., 'f16')[0] == 0x7bfe        # tie 65472 | 65504: even
    assert bits16(65489., 'f16')[0] == 0x7bff
    # the split layouts clamp both sides in fp32, the lo part stays zero
    assert bits16(1e9, 'f16x3') == (0x7bff, 0)
    assert bits16(-1e9, 'f16a2') == (0xfbff, 0)
    # hi + lo of a 21-bit integer: 0x155555 = 1398101 = 1397760 + 341
    # (hi: 11 bits 0x555 << 10 = 0x7155; lo = 341 = 0x5d54)
    # scaled by 2**-5 into the f16 range: hi = the top 11 bits 0x555 << 10,
    # lo = the other 10 bits 0x155 = 341
    assert (0x555 << 10) + 341 == 1398101
    v = torch.tensor([1398101.], dtype=torch.float32)
    hi, lo = E.split_operand(v / 32, 'f16x3', 'act')      # 43690.65625
    assert (hi.item(), lo.item()) == (43680., 10.65625)
    assert bits16(43690.65625, 'f16x3') == (0x7955, 0x4954)
    assert E.round_operand(v / 32, 'f16x3', 'act').item() == 1398101 / 32
    assert E.round_operand(v / 32, 'f16a2', 'weight').item() == 43680.
    # a Block's bias: hi + lo in the mode's type - 16 bits of a bf16 bias
    assert E.round_operand(torch.tensor([43690.]), 'bf16', 'bias').item() == 43690.
    assert bits16(43690., 'bf16', 'bias') == (0x472b, 0xc2ac)   # 43776 - 86
    # 18 bits do not fit: 174763 = 0x2aaab -> hi 171 << 10, rest -341 is the
    # tie 340 | 342 -> 340 (even)
    assert E.round_operand(
        torch.tensor([174763.]), 'bf16', 'bias').item() == 175104. - 340.
    assert E.lrelu32(torch.tensor([-30., 7., -65500.])).tolist() == [
        -3., 7., -6550.]
    assert E.quantum(torch.tensor([48., 0., -20.]).double()) == 4.
    assert E.quantum(torch.tensor([.375]).double()) == .125


# ---------------------------------------------------------------------------
# The test has teeth
# ---------------------------------------------------------------------------
def tap_conv(a, w, b, d, defect=None):
    """conv1d ('same') as a sum over taps, in float64, with one indexing
    defect planted: the wrong kernel. The first two are planted in ONE
    product of every output of the column (tap 4 / tap 2 of input channel 9),
    the unit the gates' arithmetic speaks of; the swap covers a row's k taps,
    the dilation a whole tap."""
    k, length = w.shape[-1], a.shape[-1]
    pad = d * (k - 1) // 2
    ap = F.pad(a, (pad, pad))
    w = w.clone()
    if defect == 'channels_swapped':        # two input channels, one row
        w[5, [3, 17]] = w[5, [17, 3]]
    y = b[None, :, None].expand(a.shape[0], -1, length).clone()
    for j in range(k):
        start = j * d
        if defect == 'dilation' and j == 1:     # dilation 3 taken as 2
            assert d == 3
            start = pad + (j - k // 2) * 2
        seg = ap[:, :, start:start + length].clone()
        if defect == 'neighbour_column' and j == 2:
            seg[:, 9, 64] = seg[:, 9, 63]       # at a tile boundary
        if defect == 'tap_dropped' and j == 4:
            seg[:, 9, 100] = 0.                 # one tap at one column
        y += torch.einsum('oc,bcl->bol', w[:, :, j], seg)
    return y


def defective_iteration(x, w1, b1, w2, b2, mode, d, defect):
    """block_iteration with one defect in conv1."""
    if defect in ('truncate', 'no_saturate', 'bias_unrounded'):
        flags = {'truncate': dict(truncate=True),
                 'no_saturate': dict(saturate=False),
                 'bias_unrounded': dict(round_bias=False)}[defect]
        try:
            return E.block_iteration(x, w1, b1, w2, b2, mode, d, flags)[0]
        except E.NotExact:      # (the wrong kernel need not be exact)
            return None

    def operands(a, w):
        if mode is None:
            return a.double(), w.double()
        return (E.round_operand(a, mode, 'act'),
                E.round_operand(w, mode, 'weight'))

    def bias(b):
        return b.double() if mode is None else E.round_operand(b, mode, 'bias')

    x = x.float()
    h = tap_conv(*operands(E.lrelu32(x), w1), bias(b1), d, defect)
    y = tap_conv(*operands(E.lrelu32(h.float()), w2), bias(b2), 1)
    return y + x.double()


INDEXING = ('tap_dropped', 'neighbour_column', 'channels_swapped', 'dilation')


@pytest.mark.parametrize('defect', INDEXING)
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_planted_indexing_defect(defect, mode):
    c, k, d, length = 128, 11, 3, 301
    case = E.iteration_case(mode, c, k, d, length, 0)
    # (tap_conv itself is right: no defect, same bits as the oracle)
    assert torch.equal(
        defective_iteration(case['x'], *case['w'], mode, d, None), case['want'])
    got = defective_iteration(case['x'], *case['w'], mode, d, defect)
    assert not torch.equal(got, case['want'])
    assert (got - case['want']).abs().max() >= 1.      # whole units of q
    # the same defect on the project's random-normal inputs, by the metric
    # and under the gate of test_gpu_kernels.py
    gen = torch.Generator().manual_seed(c * 100 + k)
    x = torch.randn(2, c, length, generator=gen)
    std = 1. / (c * k) ** .5
    w1 = torch.randn(c, c, k, generator=gen) * std
    w2 = torch.randn(c, c, k, generator=gen) * std
    b1 = torch.randn(c, generator=gen) * .1
    b2 = torch.randn(c, generator=gen) * .1
    want = defective_iteration(x, w1, b1, w2, b2, None, d, None)
    error = rel_err(defective_iteration(x, w1, b1, w2, b2, None, d, defect), want)
    print(f'{defect}: exact inputs differ by up to '
          f'{(got - case["want"]).abs().max().item():g} q; random-normal '
          f'inputs: rel_err {error:.2e} against the bf16 gate '
          f'{TOL_BLOCK_BF16:g}')
    assert error > 0
    if defect in ('tap_dropped', 'neighbour_column'):
        assert error < TOL_BLOCK_BF16      # (the others: module docstring)


def test_planted_rounding_defects():
    c, k, d, length = 64, 7, 3, 130
    # truncation instead of round-to-nearest-even (bf16 operands)
    case = E.iteration_case('bf16', c, k, d, length, 0)
    got = defective_iteration(case['x'], *case['w'], 'bf16', d, 'truncate')
    assert got is not None and not torch.equal(got, case['want'])
    # bf16 rounds conv1's output (thousands) - the defect must bite
    assert case['operands'][1].abs().max() > 512
    # no saturation (f16, the edge case)
    case = E.f16_edge_case('f16')
    got = defective_iteration(
        case['x'], *case['w'], 'f16', case['d'], 'no_saturate')
    # (None: an infinity reached the sums - rejected all the more)
    assert got is None or not torch.equal(got, case['want'])
    # the bias step left unrounded, with a bias beyond the 16 bits of
    # bf16 hi + lo (one bf16 alone, as one might think, would be 8)
    w1, b1, w2, b2 = E.iteration_case('bf16', 32, 3, d, length, 0)['w']
    b2 = b2.clone()                 # (conv2's: nothing rounds after it)
    b2[7] = 174763.                 # 18 bits; hi + lo = 174764
    x = E.dense_input(2, 32, length, 9)
    want, _ = E.block_iteration(x, w1, b1, w2, b2, 'bf16', d)
    got = defective_iteration(x, w1, b1, w2, b2, 'bf16', d, 'bias_unrounded')
    assert got is not None and not torch.equal(got, want)
    assert E.round_operand(b2, 'bf16', 'bias')[7].item() == 174764.


# ---------------------------------------------------------------------------
# Three iterations: the lifted cases have teeth
# ---------------------------------------------------------------------------
def forward3(x, w, mode, dilations, lo=0, length=None, truncate=False,
             plain_hidden=None):
    """A Block in float64 with no exactness check (the wrong kernel need not
    be exact) on the columns lo ... lo + x.shape[-1] of an utterance of
    `length` columns: as a tile computes it, values outside the utterance are
    zero in front of every conv, the window's own edges read zeros too.
    plain_hidden: the iteration whose hidden LeakyReLU is left out."""
    defects = dict(truncate=truncate)
    length = x.shape[-1] if length is None else length
    at = torch.arange(lo, lo + x.shape[-1])
    inside = ((at >= 0) & (at < length)).double()
    w1, b1, w2, b2 = w
    k = w1[0].shape[-1]
    y = x.double() * inside
    for n, d in enumerate(dilations):
        a = E.round_operand(E.lrelu32(y.float()), mode, 'act', **defects)
        h = F.conv1d(a, E.round_operand(w1[n], mode, 'weight', **defects),
                     E.round_operand(b1[n], mode, 'bias', **defects),
                     padding=d * (k - 1) // 2, dilation=d) * inside
        h = h.float() if n == plain_hidden else E.lrelu32(h.float())
        a = E.round_operand(h, mode, 'act', **defects)
        y = (y + F.conv1d(a, E.round_operand(w2[n], mode, 'weight', **defects),
                          E.round_operand(b2[n], mode, 'bias', **defects),
                          padding=(k - 1) // 2)) * inside
    return y


def share(got, want):
    return (got != want).double().mean().item()


LIFTED_TEETH = (('bf16', 128, 11), ('f16', 64, 7), ('fp32', 32, 3))


@pytest.mark.parametrize('mode,channels,kernel_size', LIFTED_TEETH)
def test_planted_defects_three_iterations(mode, channels, kernel_size):
    """Each defect moves a three-iteration case, by the SHARE of its elements
    that differ: what a wrong kernel would show to `torch.equal`. The floors
    are reasoned, the measured shares printed."""
    for run in range(3):
        case = E.block_case(mode, channels, kernel_size, 3, run)
        x, w, dilations, want = (
            case['x'], case['w'], case['dilations'], case['raw'])
        # (forward3 itself is right: no defect, the oracle's bits)
        assert torch.equal(forward3(x, w, mode, dilations), want)
        # the dilations of iterations 2 and 3 swapped: every output reads
        # other columns through two convs
        d = dilations
        swapped = share(forward3(x, w, mode, (d[0], d[2], d[1])), want)
        # the third iteration dropped: its conv2 adds zero only where two
        # hidden values in the thousands cancel to within the bias
        first_two = [ts[:2] for ts in w]
        dropped = share(forward3(x, first_two, mode, d[:2]), want)
        # the hidden LeakyReLU of the signed iteration left out: at least a
        # quarter of that activation is negative (asserted at build time),
        # and every row of its conv2 reads one or two elements of it
        plain = share(forward3(x, w, mode, d, plain_hidden=run), want)
        print(f'{mode} C {channels} k {kernel_size} run {run}: swapped '
              f'{swapped:.4f} dropped {dropped:.4f} no LeakyReLU in '
              f'iteration {run + 1} {plain:.4f}')
        assert swapped > .9 and dropped > .99 and plain >= .25
        # ... and left out of a LIFTED iteration it is no defect at all: the
        # construction knows which LeakyReLU each run tests
        other = (run + 1) % 3
        assert torch.equal(forward3(x, w, mode, d, plain_hidden=other), want)


def test_planted_truncation_three_iterations():
    """Round toward zero instead of to nearest even in bf16. Only values
    above 256 have more than bf16's 8 bits: with the signed iteration first
    or second they enter the second or third iteration's convs and spread
    through what follows (more than half of the outputs); with the signed
    iteration last the trunk stays below 1 600 and only the last hidden
    activation passes 256, so an output sees the defect through the two
    elements its last conv2 reads: a tenth at the least."""
    for run, floor in enumerate((.5, .5, .1)):
        case = E.block_case('bf16', 64, 7, 3, run)
        got = forward3(case['x'], case['w'], 'bf16', case['dilations'],
                       truncate=True)
        truncated = share(got, case['raw'])
        print(f'run {run}: truncation moves {truncated:.4f}')
        assert truncated > floor


def test_planted_two_iteration_halo():
    """One tile of the two-sided tiling (the bf16 C 32 k 11 geometry: 768
    columns) computed with the halo of TWO iterations instead of three: with
    the right halo the tile is the oracle's, with the short one the columns
    next to the tile's edges differ and nothing else."""
    mode, c, k, run = 'bf16', 32, 11, 0
    case = E.block_case(mode, c, k, 3, run)
    x, w, dilations, want = (
        case['x'], case['w'], case['dilations'], case['raw'])
    length = case['length']
    columns = E.block_geometry(mode, c, k)[1]
    halo = sum((d + 1) * (k - 1) // 2 for d in dilations)
    short = sum((d + 1) * (k - 1) // 2 for d in dilations[:2])
    assert (halo, short) == (60, 30)
    tile = columns - 2 * halo
    start = 3 * tile                    # an inner tile
    assert start + tile < length

    def tile_with(margin):
        lo, hi = start - margin, start + tile + margin
        y = forward3(x[:, :, lo:hi], w, mode, dilations, lo, length)
        return y[:, :, margin:margin + tile]

    assert torch.equal(tile_with(halo), want[:, :, start:start + tile])
    wrong = tile_with(short) != want[:, :, start:start + tile]
    band = halo - short
    assert not wrong[:, :, band:tile - band].any()
    edges = torch.cat([wrong[:, :, :band], wrong[:, :, tile - band:]], dim=2)
    print(f'two-iteration halo: {edges.double().mean().item():.4f} of the '
          f'{2 * band} edge columns x channels differ, '
          f'{edges.any(dim=1).double().mean().item():.4f} of the columns')
    # An output depends on its inputs along 8 chains of six taps (1 x 1,
    # 2 x 2, 1 x 2 weights per row), each chain's offset a sum of six uniform
    # taps times (1, 1, 3, 1, 5, 1): deviation 19.5 columns. An output p
    # columns inside the tile is wrong where a chain passes 30 + p columns:
    # some 6 % of the chains at p = 0, next to none at p = 29 - a few per
    # cent of the band, spread over both sides and every second column at
    # the least; one such element fails `torch.equal`.
    assert edges[:, :, 0].any() and edges[:, :, -1].any()
    assert edges.double().mean().item() >= .03
    assert edges.any(dim=1).double().mean().item() >= .25
