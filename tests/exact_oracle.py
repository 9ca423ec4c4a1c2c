"""Oracle and inputs for the EXACT tests of the conv kernels
(test_gpu_exact.py, test_cpu_exact_oracle.py).

The inputs are chosen so that every product and every partial sum of a conv is
an integer multiple of one quantum q and stays below 2**22 q: such a sum is
exactly representable in fp32 whatever the order of summation, so the kernels
are compared with `torch.equal` against float64, with no tolerance. A wrong
index, tap, column, channel, dilation, rounding mode or a stale byte moves an
output by whole units of q.

One iteration runs dense, two sparse (sparse_block), three lifted
(lifted_block: what keeps three iterations inside the bound is said there).

Everything here restates what the kernels do to a value, read from the code:

  activations  cvt(pm_lrelu(v)), pm_lrelu(v) = fmax(v, v * 0.1f) in fp32
               (pm_common.h); cvt is round-to-nearest-even. f16 converts and
               then takes min(., 65504) - the upper side only (ElemF16::store4);
               the split layouts clamp to +-65504 in fp32 first
               (ElemF16X3::split4), hi = f16(v'), lo = f16(v' - hi).
  weights      cvt(w), not clamped; f16x3: hi + lo; f16a2: f16 once.
  biases       Block kernels: a bias step of the weight stream
               (pm_pack_bias_step_kernel), T(b) + T(b - T(b)) in the 16-bit
               type T of the mode - twice the type's precision, not once -,
               fp32: b itself. Upsampler / input conv: fp32 in the epilogue,
               never rounded.
  f16x3        hi.hi + hi.lo + lo.hi, lo.lo dropped: inputs where both factors
               of a product have a lo part are outside the exact domain and
               assert.
  accumulation fp32 everywhere.
"""
import functools
import math

import torch
import torch.nn.functional as F

MODES = ('fp32', 'f16', 'bf16', 'f16x3', 'f16a2')
F16_MAX = 65504.
# bits of bound / q a conv may reach: fp32 holds 24, two are left to the
# matrix unit's internal alignment of the products of one instruction
EXACT_BITS = 22

_SLOPE = torch.tensor(.1, dtype=torch.float32)


def lrelu32(v):
    assert v.dtype == torch.float32
    return torch.maximum(v, v * _SLOPE)


def _cast(v, dtype):
    return v.to(dtype).to(torch.float32)


def split_operand(v, mode, role, truncate=False, saturate=True,
                  round_bias=True):
    """(hi, lo) float64 parts of what the kernel feeds the matrix unit for
    the fp32 tensor `v`; role: 'act', 'weight' or 'bias' (a Block's bias
    step). `truncate`, `saturate` and `round_bias` exist to plant defects
    (test_cpu_exact_oracle.py) and are never set by the oracle itself."""
    assert v.dtype == torch.float32 and mode in MODES
    assert role in ('act', 'weight', 'bias')
    zero = torch.zeros_like(v)
    half = torch.bfloat16 if mode == 'bf16' else torch.float16

    def cvt(t):
        if not truncate:
            return _cast(t, half)
        # round toward zero: clear the mantissa bits the type drops
        assert half == torch.bfloat16
        return (t.view(torch.int32) & ~0xffff).view(torch.float32)

    if mode == 'fp32':
        hi, lo = v, zero
    elif role == 'bias':
        if not round_bias:
            hi, lo = v, zero
        else:
            hi = cvt(v)
            lo = cvt(v - hi)
    elif role == 'weight':
        hi = cvt(v)
        lo = cvt(v - hi) if mode == 'f16x3' else zero
    elif mode == 'bf16':
        hi, lo = cvt(v), zero
    elif mode == 'f16':
        hi, lo = cvt(v), zero
        if saturate:
            hi = hi.clamp(max=F16_MAX)
    else:
        w = v.clamp(-F16_MAX, F16_MAX) if saturate else v
        hi = cvt(w)
        lo = cvt(w - hi)
    return hi.double(), lo.double()


def round_operand(v, mode, role, **defects):
    hi, lo = split_operand(v, mode, role, **defects)
    return hi + lo


class NotExact(AssertionError):
    pass


def quantum(*tensors):
    """Smallest value of the lowest set mantissa bit over the non-zero
    elements of float64 tensors (inf if all are zero)."""
    q = math.inf
    for t in tensors:
        t = t[t != 0]
        if t.numel() == 0:
            continue
        if not torch.isfinite(t).all():
            raise NotExact('an operand is not finite')
        mant, exp = torch.frexp(t.double())
        bits = (mant.abs() * 2. ** 53).to(torch.int64)
        low = bits & -bits
        q = min(q, (low.double() * torch.exp2(exp.double() - 53)).min().item())
    return q


def exactness(result, bound, q):
    """Bits of bound / q; raises unless the conv that gave `result` (float64)
    is exact in fp32 whatever the order of summation."""
    if bound == 0 or q == math.inf:
        return 0.
    bits = math.log2(bound / q)
    if not bits <= EXACT_BITS:
        raise NotExact(f'{bits:.1f} bits > {EXACT_BITS}')
    if not torch.equal(result.float().double(), result):
        raise NotExact('result does not fit fp32')
    return max(bits, 0.)


def _operands(a32, w32, mode, defects):
    ahi, alo = split_operand(a32, mode, 'act', **defects)
    whi, wlo = split_operand(w32, mode, 'weight', **defects)
    # lo x lo is dropped by the kernel: not in the exact domain
    assert not (alo.any() and wlo.any()), 'lo x lo product'
    return ahi + alo, whi + wlo, quantum(ahi, alo) * quantum(whi, wlo)


def conv(a32, w32, b64, mode, dilation=1, residual=None, defects=None):
    """Conv1d ('same') of the operands of fp32 activations `a32` (after
    LeakyReLU where the kernel applies one) and weights `w32`, + b64
    (+ residual, which the kernels hold in the accumulator), in float64.
    Returns (result, bits)."""
    a, w, q = _operands(a32, w32, mode, defects or {})
    k = w.shape[-1]
    pad = dilation * (k - 1) // 2
    y = F.conv1d(a, w, b64, padding=pad, dilation=dilation)
    bound = F.conv1d(a.abs(), w.abs(), b64.abs(), padding=pad,
                     dilation=dilation)
    if residual is not None:
        y = y + residual
        bound = bound + residual.abs()
        q = min(q, quantum(residual))
    q = min(q, quantum(b64))
    return y, exactness(y, bound.max().item(), q)


def store(y, mode=0, scale=1., out=None):
    """The store modes of the Block kernels: 0 out = y, 1 out = y * scale,
    2 out += y * scale (scale a power of two: the same bits fused or not)."""
    assert math.frexp(scale)[0] == .5
    if mode == 0:
        return y
    r = y * scale if mode == 1 else out.double() + y * scale
    if not torch.equal(r.float().double(), r):
        raise NotExact('stored value does not fit fp32')
    return r


def block_iteration(x, w1, b1, w2, b2, mode, d, defects=None):
    """One Block iteration (pm_block_iteration_cl before its store mode):
    x + conv2(lrelu(conv1(lrelu(x)))). fp32 tensors in, (float64, bits) out."""
    defects = defects or {}
    x = x.float()
    h, bits1 = conv(lrelu32(x), w1, round_operand(b1, mode, 'bias', **defects),
                    mode, d, None, defects)
    y, bits2 = conv(lrelu32(h.float()), w2,
                    round_operand(b2, mode, 'bias', **defects), mode, 1,
                    x.double(), defects)
    return y, max(bits1, bits2)


def block(x, w1, b1, w2, b2, mode, dilations, defects=None):
    """A Block of len(dilations) iterations (pm_block_cl before its store
    mode); w1 ... b2 are lists, one entry per iteration."""
    bits = 0.
    y = x.double()
    for n, d in enumerate(dilations):
        y, b = block_iteration(
            y.float(), w1[n], b1[n], w2[n], b2[n], mode, d, defects)
        bits = max(bits, b)
    return y, bits


def mrf_sum(x, blocks, mode, dilations):
    """pm_mrf_cl before its final * (1 / 3): the Blocks' results (a list)
    and their exact sum S; blocks = [(w1, b1, w2, b2), ...] for k 3, 7, 11."""
    parts, bits = [], 0.
    for w1, b1, w2, b2 in blocks:
        y, b = block(x, w1, b1, w2, b2, mode, dilations)
        parts.append(y)
        bits = max(bits, b)
    total = sum(parts)
    if not torch.equal(total.float().double(), total):
        raise NotExact('the MRF sum does not fit fp32')
    return parts, total, bits


def conv_transpose(x, w, bias, mode, rate, staged=False):
    """lrelu -> ConvTranspose1d(k = 2 rate, stride rate, pad rate / 2)
    (pm_conv_transpose_cl with lrelu = 1); the bias is added in fp32.
    staged: `x` already holds the operand values (pm_conv_transpose_x16_cl)."""
    a32 = x.float() if staged else lrelu32(x.float())
    a, wr, q = _operands(a32, w, mode, {})
    k = w.shape[-1]
    args = dict(stride=rate, padding=(k - rate) // 2)
    y = F.conv_transpose1d(a, wr, bias.double(), **args)
    bound = F.conv_transpose1d(a.abs(), wr.abs(), bias.double().abs(), **args)
    q = min(q, quantum(bias.double()))
    return y, exactness(y, bound.max().item(), q)


def input_conv(x, w, bias, g, sw, sb, mode):
    """Conv1d(k 7, pad 3) of the features (no LeakyReLU) + the speaker conv
    (k 1) of the globals as a per-utterance fp32 bias (pm_input_conv_cl);
    g (1 | B, G)."""
    a, wr, q = _operands(x.float(), w, mode, {})
    gb = F.linear(g.double(), sw.double()[:, :, 0], sb.double())    # fp32 FMAs
    gbound = F.linear(g.double().abs(), sw.double()[:, :, 0].abs(),
                      sb.double().abs())
    bits = exactness(gb, gbound.max().item(),
                     min(quantum(g.double()) * quantum(sw.double()),
                         quantum(sb.double())))
    every = (bias.double()[None] + gb)[:, :, None]
    y = F.conv1d(a, wr, None, padding=3) + every
    bound = F.conv1d(a.abs(), wr.abs(), None, padding=3) + every.abs()
    q = min(q, quantum(every))
    return y, max(bits, exactness(y, bound.max().item(), q))


# ---------------------------------------------------------------------------
# Input builders (seeded)
# ---------------------------------------------------------------------------
def _choice(values, shape, gen):
    values = torch.tensor(values, dtype=torch.float32)
    return values[torch.randint(len(values), shape, generator=gen)]


DENSE_X = tuple(range(1, 9)) + tuple(-10 * m for m in range(9))


def dense_iteration(c, k, seed):
    """Weights of one dense iteration: w1 in 10 {-2..2}, b1 in 10 {-9..9},
    w2 in {-2..2}, b2 in {-9..9}. With x from DENSE_X, fmax(v, v * 0.1f) is
    an integer for every operand (checked in fp32 by the CPU test): all
    operands have quantum >= 1."""
    gen = torch.Generator().manual_seed(seed)
    # (beyond 1792 products a sum - C 256 k 11 - {-2..2} passes 22 bits in
    # conv2: sqrt(C k) grows the operands, C k the bound)
    values = range(-2, 3) if c * k <= 1792 else range(-1, 2)
    w1 = 10 * _choice(values, (c, c, k), gen)
    b1 = 10 * _choice(range(-9, 10), (c,), gen)
    w2 = _choice(values, (c, c, k), gen)
    b2 = _choice(range(-9, 10), (c,), gen)
    return w1, b1, w2, b2


def dense_input(batch, c, length, seed):
    gen = torch.Generator().manual_seed(seed)
    return _choice(DENSE_X, (batch, c, length), gen)


def sparse_weight(c, k, gen, phase):
    """(c, c, k) with two non-zeros 10 {+-1} per output row. The 2 c
    positions (c_in, tap) are a run of a seeded permutation of all c k
    positions that starts at 2 c phase: over ceil(k / 2) consecutive phases
    every position is non-zero once."""
    positions = c * k
    order = torch.randperm(positions, generator=torch.Generator().manual_seed(
        c * 1000 + k))
    w = torch.zeros(c, positions)
    rows = torch.arange(c)
    for j in range(2):
        at = order[(2 * c * phase + 2 * rows + j) % positions]
        w[rows, at] = 10 * _choice((-1, 1), (c,), gen)
    return w.view(c, c, k)


def sparse_block(c, k, niter, seed, phase):
    """Weights of `niter` sparse iterations: every weight 10 {+-1}, two per
    output row; biases 10 {-1, 0, 1}. Values grow by at most 20 x a conv."""
    gen = torch.Generator().manual_seed(seed)
    out = ([], [], [], [])
    for _ in range(niter):
        for which in (0, 2):
            out[which].append(sparse_weight(c, k, gen, phase))
            out[which + 1].append(10 * _choice((-1, 0, 1), (c,), gen))
    return out


def sparse_input(batch, c, length, seed):
    gen = torch.Generator().manual_seed(seed)
    return 10 * _choice((-1, 0, 1), (batch, c, length), gen)


# Three iterations. sparse_block multiplies by 10 at every conv so that the
# values stay multiples of 10 for v * 0.1f: 20 x a conv, 20**6 over three
# iterations. A lifted Block pays that in ONE iteration, the signed one:
#
#   signed   conv1 one weight 10 {+-1} per row, bias 10 {-1, 0, 1}: the hidden
#            activation is a multiple of 10 of both signs; conv2 10 {+-1}.
#   lifted   conv1 weights +1 and a constant bias, the lift, no smaller than
#            the weights per row times the largest |negative| operand the
#            trunk can hand it: the hidden activation is >= 0, its LeakyReLU
#            the identity, and it is an integer whatever the operand rounding
#            did to the trunk. conv2 10 {+-1}, bias 10 {-1, 0, 1}: the trunk
#            stays a multiple of 10 of both signs.
#   the Block's last conv2: {+-1}, bias -9..9 - no LeakyReLU follows.
#
# LIFTED_ROWS[position of the signed iteration] = weights per row of
# (conv1, conv2) per iteration, chosen so that the WORST case of every
# operand (lifted_block walks it) stays under 65504 with bf16's rounding on
# top; the cases assert what they actually reach.
LIFTED_ROWS = {0: ((1, 2, 1), (1, 2, 2)),
               1: ((2, 1, 1), (1, 2, 2)),
               2: ((1, 1, 1), (1, 1, 2))}


def _ceil_bits(v, bits):
    """The smallest integer >= v with at most `bits` significant bits."""
    v = int(math.ceil(v))
    shift = max(v.bit_length() - bits, 0)
    return -(-v // (1 << shift)) << shift


def lifted_weight(c, k, per_row, values, gen):
    """(c, c, k) with `per_row` non-zeros from `values` per output row, and
    every input channel and every tap non-zero (c >= k): weight j of row r
    reads input channel p[(r + j) % c] at tap t[(r + 3 j) % k], p and t drawn
    from `gen`. (A run of a permutation of all c k positions, as
    sparse_weight takes it, leaves input channels out at one weight per
    row.)"""
    assert per_row <= 3 <= k <= c
    p, t = torch.randperm(c, generator=gen), torch.randperm(k, generator=gen)
    values = torch.tensor(values, dtype=torch.float32)
    w = torch.zeros(c, c, k)
    rows = torch.arange(c)
    for j in range(per_row):
        # (as many rows of one value as of the other: with one weight per
        # row its sign is the sign of the whole output row)
        w[rows, p[(rows + j) % c], t[(rows + 3 * j) % k]] = \
            values[torch.randperm(c, generator=gen) % len(values)]
    return w


def lifted_block(c, k, seed, signed):
    """Weights of three iterations, the `signed`-th signed and the others
    lifted (above), and the worst case of |operand| in front of each of the
    six convs."""
    gen = torch.Generator().manual_seed(seed)
    n1, n2 = LIFTED_ROWS[signed]
    out, worst = ([], [], [], []), []
    trunk = 10                          # sparse_input
    for n in range(3):
        worst.append(trunk)
        if n == signed:
            out[0].append(lifted_weight(c, k, n1[n], (-10, 10), gen))
            out[1].append(10 * _choice((-1, 0, 1), (c,), gen))
            hidden = 10 * n1[n] * trunk + 10
        else:
            # the largest negative operand: trunk / 10, rounded away from
            # zero to bf16's 8 bits at the most
            lift = _ceil_bits(n1[n] * _ceil_bits(trunk / 10, 8), 4)
            out[0].append(lifted_weight(c, k, n1[n], (1,), gen))
            out[1].append(torch.full((c,), float(lift)))
            hidden = n1[n] * trunk + lift
        worst.append(hidden)
        if n == 2:
            out[2].append(lifted_weight(c, k, n2[n], (-1, 1), gen))
            out[3].append(_choice(range(-9, 10), (c,), gen))
        else:
            out[2].append(lifted_weight(c, k, n2[n], (-10, 10), gen))
            out[3].append(10 * _choice((-1, 0, 1), (c,), gen))
            trunk = trunk + 10 * n2[n] * _ceil_bits(hidden, 8) + 10
    assert max(worst) * (1 + 2. ** -8) < F16_MAX, worst
    return out, worst


def lifted_operands(x, w, mode, dilations):
    """fp32 values in front of every conv of a Block (before LeakyReLU and
    operand rounding): trunk, hidden, trunk, hidden, ..."""
    out = []
    y = x.double()
    w1, b1, w2, b2 = w
    for n, d in enumerate(dilations):
        h, _ = conv(lrelu32(y.float()), w1[n],
                    round_operand(b1[n], mode, 'bias'), mode, d)
        out += [y.float(), h.float()]
        y, _ = conv(lrelu32(h.float()), w2[n],
                    round_operand(b2[n], mode, 'bias'), mode, 1, y)
    return out


def first_accepted(draw, draws=4):
    """draw(0), or the first of the next draws that meets its conditions: a
    short case (one column: all taps but the centre read padding) can miss a
    share of negative values by chance. The conditions stay as they are."""
    for n in range(draws):
        try:
            return draw(n)
        except NotExact as error:
            refused = error
    raise refused


def assert_lifted(x, w, mode, dilations, signed):
    """The conditions of a three-iteration case (NotExact otherwise); returns
    the largest operand."""
    before = lifted_operands(x, w, mode, dilations)
    largest = max(lrelu32(t).abs().max().item() for t in before)
    if not largest < F16_MAX:       # in EVERY mode: no clamp makes a case pass
        raise NotExact(f'operand {largest:g} >= {F16_MAX:g}')
    for n in range(3):
        trunk, hidden = before[2 * n], before[2 * n + 1]
        if not (trunk < 0).float().mean() >= .25:
            raise NotExact(f'trunk of iteration {n} negative in < 25 %')
        if n == signed:
            if not (hidden < 0).float().mean() >= .25:
                raise NotExact('signed hidden activation negative in < 25 %')
        elif not (hidden >= 0).all():
            raise NotExact(f'lifted hidden activation of iteration {n} < 0')
    for weight in w[0] + w[2]:
        hit = weight != 0
        if not (hit.any(dim=(0, 2)).all() and hit.any(dim=(0, 1)).all()):
            raise NotExact('an input channel or a tap without a weight')
    return largest


def int_fill(batch, c, length, seed):
    """A pre-filled `out` (store mode 2): integers in -99..99."""
    gen = torch.Generator().manual_seed(seed)
    return _choice(range(-99, 100), (batch, c, length), gen)


# ---------------------------------------------------------------------------
# The case table: the GPU tests take their cases from here, the CPU test
# builds every one and asserts that it is exact
# ---------------------------------------------------------------------------
BATCH = 2
SCALES = {0: 1., 1: .5, 2: .25}

# (a) pm_block_iteration_cl
ITERATION_CHANNELS = (32, 64, 128, 256, 8, 48)
ITERATION_KERNELS = (3, 7, 11)
# (dilation, length, store mode): every d with every L class - shorter than
# the halo, one past a tile, ragged - and the three store modes
ITERATION_RUNS = tuple(
    (d, length, (i + j) % 3)
    for i, d in enumerate((1, 3, 5))
    for j, length in enumerate((1, 9, 130, 301)))


@functools.lru_cache(maxsize=None)
def iteration_case(mode, c, k, d, length, store_mode):
    w = dense_iteration(c, k, 7 * c + k)
    x = dense_input(BATCH, c, length, 100 * c + 10 * k + d)
    prev = int_fill(BATCH, c, length, length + d)
    y, bits = block_iteration(x, *w, mode, d)
    want = store(y, store_mode, SCALES[store_mode], prev)
    return dict(x=x, w=w, prev=prev, want=want, bits=bits,
                operands=iteration_operands(x, w, mode, d))


# The pair kernel's WIDE geometry (PairCfg of pm_launch.h; C = 128 / 256 take
# PairCfgNarrow below 150 workgroups, which is every length above): batch 2 x
# 76 tiles of 256 - (k - 1) / 192 - (k - 1) columns, 16-bit operands, k 3
ITERATION_WIDE = ((128, 3, 75 * 254 + 7), (256, 3, 75 * 190 + 7))


def iteration_wide_case(mode, c):
    k, length = {c_: (k_, l_) for c_, k_, l_ in ITERATION_WIDE}[c]
    return iteration_case(mode, c, k, 3, length, 2)


def iteration_operands(x, w, mode, d):
    """fp32 activations of both convs before the operand rounding (the f16
    range check of the CPU test)."""
    a1 = lrelu32(x)
    h, _ = conv(a1, w[0], round_operand(w[1], mode, 'bias'), mode, d)
    return a1, lrelu32(h.float())


# (b), (c) pm_block_cl. Shapes: test_gpu_kernels.py's SKEW_SHAPES, which
# hold the walked list
BLOCK_SHAPES = ((32, 3), (32, 7), (32, 11), (64, 3), (64, 7), (64, 11),
                (128, 3), (128, 7), (128, 11), (256, 3), (256, 7))
# the Block3Cfg geometries of pm_launch.h: waves (WM WN) and columns of a
# tile (32 WN NTW), 16-bit and 4-byte operand layouts
_GEOMETRY16 = {(32, 3): (4, 384), (32, 7): (4, 384), (32, 11): (8, 768),
               (64, 3): (4, 256), (64, 7): (8, 512), (64, 11): (8, 512),
               (128, 3): (8, 256), (128, 7): (8, 256), (128, 11): (8, 256),
               (256, 3): (8, 128), (256, 7): (8, 128)}
_GEOMETRY32 = {(32, 3): (8, 512), (32, 7): (8, 512), (32, 11): (8, 512),
               (64, 3): (8, 256), (64, 7): (8, 256), (64, 11): (8, 256)}


def block_geometry(mode, c, k):
    table = _GEOMETRY16 if mode in ('f16', 'bf16') else _GEOMETRY32
    return table.get((c, k))


def block_form(mode, c, k, request):
    """The kernel pm_block_cl takes for `request` ('own': the launcher's
    choice at these lengths; 'walked': pm_debug_force(nseg), no scratch;
    'skewed': pm_debug_force(nseg), pm_debug_skew(1), scratch handed over),
    from Block3Kernels / plan_block_cfg of pm_launch.h; None: no kernel."""
    geometry = block_geometry(mode, c, k)
    if geometry is None:
        return None
    waves, _ = geometry
    wide = mode not in ('f16', 'bf16')
    skew = waves == 8
    walk = waves == 8 and not wide and (c, k) not in ((128, 11), (256, 7))
    tiled = not (c == 128 and k >= 7) and c != 256
    if request == 'skewed':
        return 'skewed' if skew else None
    if request == 'walked':
        return 'walked' if walk else None
    return 'tiled' if tiled else None


def block_requests(mode, c, k):
    return [r for r in ('own', 'walked', 'skewed')
            if block_form(mode, c, k, r)]


def block_runs(mode, c, k, niter):
    """(nseg, length, dilations, store mode) of a Block case: 2 and 3
    segments, uneven, a boundary that is no tile multiple, an utterance end
    inside a tile, an utterance shorter than the halo / the skew."""
    columns = block_geometry(mode, c, k)[1]
    if niter == 1:
        dilations = ((1,), (3,), (5,))
    elif niter == 2:
        dilations = ((1, 3), (3, 5), (5, 1))
    else:
        # (61: shorter than the 64-column skew of three iterations, one more
        # than their halo at k 11; every rotation passes pm_skew_dilations)
        dilations = ((1, 3, 5), (3, 5, 1), (5, 1, 3))
    return ((2, 9 * columns + 37, dilations[0], 0),
            (3, 2 * columns + 1, dilations[1], 2),
            (2, 61, dilations[2], 1))


def block_modes(c):
    return MODES if c <= 64 else ('f16', 'bf16')


def block_phase(mode, c, k, run):
    """Coverage phase of a sparse case: consecutive over the cases of (c, k)."""
    return block_modes(c).index(mode) * 3 + run


@functools.lru_cache(maxsize=None)
def block_case(mode, c, k, niter, run):
    nseg, length, dilations, store_mode = block_runs(mode, c, k, niter)[run]
    seed = 1000 * c + 10 * k + run
    extra = {}
    if niter == 1:
        w = tuple([t] for t in dense_iteration(c, k, seed))
        x = dense_input(BATCH, c, length, seed + 1)
    elif niter == 2:
        w = sparse_block(c, k, niter, seed, block_phase(mode, c, k, run))
        x = sparse_input(BATCH, c, length, seed + 1)
    else:
        # the signed iteration is the run's: over the runs of a shape every
        # iteration's hidden LeakyReLU sees negative values; the weight
        # positions are drawn anew for every case of (c, k)
        def draw(n):
            w, worst = lifted_block(
                c, k, seed + 100003 * block_phase(mode, c, k, run) + 977 * n,
                run)
            x = sparse_input(BATCH, c, length, seed + 1 + 977 * n)
            return x, w, dict(
                signed=run, worst=worst,
                largest=assert_lifted(x, w, mode, dilations, run))
        x, w, extra = first_accepted(draw)
    prev = int_fill(BATCH, c, length, seed + 2)
    y, bits = block(x, *w, mode, dilations)
    want = store(y, store_mode, SCALES[store_mode], prev)
    return dict(x=x, w=w, prev=prev, want=want, bits=bits, raw=y, nseg=nseg,
                length=length, dilations=dilations, store_mode=store_mode,
                **extra)


def block_table():
    """(mode, c, k, niter) of every Block case of (b) and (c)."""
    return [(mode, c, k, niter) for niter in (1, 2, 3) for c, k in BLOCK_SHAPES
            for mode in block_modes(c)]


# (d) pm_mrf_cl
MRF_CHANNELS = (32, 20)
MRF_LENGTHS = (1, 61, 700, 3000)
MRF_DILATIONS = {1: ((1,), (3,), (5,), (3,)), 2: ((1, 3), (3, 5), (5, 1), (1, 3)),
                 3: ((1, 3, 5), (3, 5, 1), (5, 1, 3), (1, 3, 5))}


def mrf_lengths(mode, niter):
    """Three iterations reach the walked and the skewed whole-MRF kernels
    (plan_mrf_cfg): in columns NC of the k 11 geometry they run on, shorter
    than a tile, the skew and the halo's neighbour 61, 2 NC + 1 - 3 segments
    take less than a tile each -, 5 NC + 37 - uneven segments, ragged ends."""
    if niter < 3:
        return MRF_LENGTHS
    columns = block_geometry(mode, 32, 11)[1]
    return (1, 61, 2 * columns + 1, 5 * columns + 37)


@functools.lru_cache(maxsize=None)
def mrf_case(mode, c, niter, run):
    length = mrf_lengths(mode, niter)[run]
    dilations = MRF_DILATIONS[niter][run]
    def draw(n):
        blocks, extra = [], {}
        x = (dense_input if niter == 1 else sparse_input)(
            BATCH, c, length, 77 * c + run + 977 * n)
        for k in (3, 7, 11):
            seed = 500 * c + 10 * k + run + 977 * n
            if niter == 1:
                blocks.append(tuple([t] for t in dense_iteration(c, k, seed)))
            elif niter == 2:
                blocks.append(sparse_block(c, k, niter, seed, run))
            else:
                # (the three Blocks' signed iteration is the same one)
                w, _ = lifted_block(c, k, seed, run % 3)
                blocks.append(w)
                extra = dict(signed=run % 3, largest=max(
                    extra.get('largest', 0.),
                    assert_lifted(x, w, mode, dilations, run % 3)))
        return x, blocks, extra
    # (one and two iterations have no conditions to miss: draw(0) as ever)
    x, blocks, extra = first_accepted(draw) if niter == 3 else draw(0)
    parts, total, bits = mrf_sum(x, blocks, mode, dilations)
    return dict(x=x, blocks=blocks, parts=parts, total=total, bits=bits,
                length=length, dilations=dilations, **extra)


# (e) the upsamplers: test_conv_transpose's shapes
UPSAMPLE_SHAPES = ((512, 256, 8), (256, 128, 8), (128, 64, 2), (64, 32, 2),
                   (64, 32, 8), (32, 16, 2), (16, 8, 4))
UPSAMPLE_LENGTHS = (1, 5, 130, 300)
# The c_in 128 r = 2 upsampler with 16-bit operands takes 256 input columns a
# workgroup, not 128, from batch * ceil(length / 256) >= 1024 on (batch is the
# cheap axis): one mostly empty tile per utterance; a full and a ragged tile,
# exactly at the threshold; one utterance fewer, the 128-column side of the
# rule on the same data (the first 511 utterances of the 512).
# (batch, length, batch drawn)
UPSAMPLE_LONG = ((1024, 5, 1024), (512, 300, 512), (511, 300, 512))


@functools.lru_cache(maxsize=None)
def upsample_case(mode, c_in, c_out, rate, length, batch=BATCH):
    gen = torch.Generator().manual_seed(c_in + 10 * rate + length)
    x = 10 * _choice(range(-9, 10), (batch, c_in, length), gen)
    w = _choice(range(-3, 4), (c_in, c_out, 2 * rate), gen)
    bias = _choice(range(-999, 1000), (c_out,), gen)
    y, bits = conv_transpose(x, w, bias, mode, rate)
    return dict(x=x, w=w, bias=bias, want=y, bits=bits)


@functools.lru_cache(maxsize=1)     # (hundreds of MB: one at a time)
def upsample_long_case(mode, length, drawn):
    return upsample_case.__wrapped__(mode, 128, 64, 2, length, drawn)


# (f) the f16 operand edge: activations at 65504, on both sides of the last
# rounding boundary below it (65488, the tie between 65472 and 65504), on
# both sides of the boundary to infinity (65520) and far above
F16_EDGE = (65504., 65487., 65488., 65489., 65519., 65520., 65521., 65536.,
            70000., 300000., 3000000.)


@functools.lru_cache(maxsize=None)
def f16_edge_case(mode):
    c, k, d, length = 32, 7, 3, 130
    gen = torch.Generator().manual_seed(65504)
    # two weights per row: two saturated operands stay inside the bound.
    # conv1 is non-negative (w1 = 1, b1 >= 0, x >= 0), so that no negative
    # value that is no multiple of 10 meets v * 0.1f
    w1 = torch.zeros(c, c, k)
    w2 = torch.zeros(c, c, k)
    for w, signs in ((w1, (1,)), (w2, (-1, 1))):
        rows = torch.arange(c)
        for _ in range(2):
            w[rows, torch.randint(c, (c,), generator=gen),
              torch.randint(k, (c,), generator=gen)] = _choice(signs, (c,), gen)
    b1 = _choice(range(0, 10), (c,), gen)
    b2 = _choice(range(-9, 10), (c,), gen)
    x = _choice(range(0, 9), (1, c, length), gen)
    at = torch.randperm(c * length, generator=gen)[:4 * len(F16_EDGE)]
    x.view(-1)[at] = torch.tensor(F16_EDGE * 4)
    y, bits = block_iteration(x, w1, b1, w2, b2, mode, d)
    return dict(x=x, w=(w1, b1, w2, b2), want=y, bits=bits, k=k, d=d)


# (g) pm_input_conv_cl: test_input_conv's shapes (c_in, c_out, G)
INPUT_SHAPES = ((113, 512, 258), (113, 64, 258), (40, 32, 6))
INPUT_RUNS = ((2, 45, 2), (3, 130, 1), (3, 1, 3))   # batch, length, gbatch
INPUT_MODES = ('fp32', 'f16', 'f16x3', 'f16a2')     # (no bf16 input layer)


@functools.lru_cache(maxsize=None)
def input_case(mode, c_in, c_out, G, run):
    batch, length, gbatch = INPUT_RUNS[run]
    gen = torch.Generator().manual_seed(c_in + c_out + run)
    w = _choice(range(-3, 4), (c_out, c_in, 7), gen)
    bias = _choice(range(-99, 100), (c_out,), gen)
    sw = _choice(range(-3, 4), (c_out, G, 1), gen)
    sb = _choice(range(-99, 100), (c_out,), gen)
    x = _choice(range(-64, 65), (batch, c_in, length), gen)
    g = _choice(range(-9, 10), (gbatch, G), gen)
    y, bits = input_conv(x, w, bias, g, sw, sb, mode)
    return dict(x=x, w=w, bias=bias, sw=sw, sb=sb, g=g, want=y, bits=bits)


def first_difference(got, want, q=1.):
    """Where two (B, C, L) tensors first differ, for a failure message."""
    diff = (got.double() != want.double()).nonzero()
    if diff.numel() == 0:
        return 'equal'
    b, c, t = diff[0].tolist()
    g, w = got[b, c, t].item(), want[b, c, t].item()
    return (f'{diff.shape[0]} of {want.numel()} differ; first at batch {b} '
            f'column {t} channel {c}: got {g!r} want {w!r} '
            f'({(g - w) / q:+g} q, q = {q:g})')
