"""Oracle and inputs for the EXACT tests of the Vocos kernels
(test_gpu_vocos_exact.py, test_cpu_vocos_exact.py): vocos_block_kernel and
vocos_gemm_kernel of pm_vocos.h against float64 with `torch.equal`.

The ConvNeXt block holds a LayerNorm and a GELU; the inputs make both exact.

  depthwise conv  channel c has ONE non-zero tap tau(c), of weight +-1, and no
                  bias; x = 8 s sign(w) with s = +-1 balanced within every tap
                  class of every row. Every conv output is +-8 or, where the
                  tap falls outside the utterance, 0; a wrong tap, a wrong row
                  or a halo read across an utterance end is another pattern.
  LayerNorm       the mean is exactly 0 and the variance n / 8 for n live
                  channels (fp32 sums of integers). INTERIOR rows
                  (3 <= t < T - 3): 64 + 1e-6f is 64 in fp32 and rstd is 1 / 8
                  up to the device's last ulp, which the cast to the 16-bit
                  type absorbs: +-g + beta with g odd and beta even is an odd
                  integer, never 0 (a residue of 1e-7 would survive in bf16)
                  and never at a rounding tie. EDGE rows: rstd is irrational;
                  the oracle takes xn in float64, rounds it to the type and
                  asserts that every value is at least TIE_MARGIN (relative,
                  16 fp32 ulps) away from a rounding tie and, where it is not
                  exactly zero, at least 0.5 in size.
  GELU            b1 = +-(16 + the bound of the row's contraction): every
                  pre-activation has |v| >= 16, where erf is +-1 in any
                  implementation; 0.5f v (1 + 1) is v and 0.5f v 0 is -0. The
                  oracle uses ReLU and asserts the condition.
  contractions    W1 and W2 are sparse +-1, b2 integer, gamma a power of two:
                  `quantum` / `exactness` of exact_oracle.py hold both
                  contractions and the epilogue to EXACT_BITS. The bias add
                  v = c1 + b1 is one fp32 addition, exact when v fits fp32
                  (asserted). h = cvt(v) is a rounding of an exactly known
                  value: deterministic, ties included, and where a wrong
                  rounding mode shows. A few channels have g = 515 (xn that
                  bf16 cannot hold, no tie: its grid there is 4) and a few
                  hidden units b1 beyond 2048 (h that f16 cannot hold).

What the kernel does to a value, restated (vocos_block_kernel,
vc_layer_norm8): fp32 fmaf over the taps, bias added last; mean subtracted
before the squares; rstd = 1.f / sqrtf(var + 1e-6f);
xn = cvt(v rstd g + beta); h = cvt(gelu(c1 + b1)); y = x + gamma (acc + b2);
cvt a plain cast, round to nearest even, no saturation (operands above 65504
are outside the f16 domain and assert).

fp32 mode is not bit-exact (rstd's last ulp reaches the output): the oracle
derives a per-element bound by propagating a relative error RSTD_ERROR in
rstd through |W1|, |W2| and gamma and, on edge rows, one fp32 rounding
(2**-24 relative) per operation. Nothing in it is measured.

What these inputs cannot see: the SHAPE of GELU (a tanh approximation is
identical where |v| >= 16) and LayerNorm on generic rows (mean and variance
that are not exact). Those stay with the fp32 gate of test_gpu_vocos.py.
"""
import functools

import torch
import torch.nn.functional as F

import exact_oracle as E
from exact_oracle import NotExact, exactness, quantum

MODES = ('fp32', 'f16', 'bf16')
HALF = {'f16': torch.float16, 'bf16': torch.bfloat16}
PRECISION = {'f16': 11, 'bf16': 8}          # significand bits
CHANNELS = 512                              # PM_VOCOS_C
CHUNK = 64                                  # PM_VOCOS_HC
TIE_MARGIN = 2. ** -20
RSTD_ERROR = 2. ** -22
U = 2. ** -24                               # one fp32 rounding, relative
_EPS = torch.tensor(1e-6, dtype=torch.float32)


def cvt(v32, mode, truncate=False):
    """ET::cvt of fp32 values, as float64: the plain cast exact_oracle.py
    applies to weights (no clamp). `truncate` plants a defect (round toward
    zero) and is never set by the oracle."""
    assert v32.dtype == torch.float32 and mode in MODES
    if mode == 'fp32':
        return v32.double()
    if not truncate:
        return E.round_operand(v32, mode, 'weight')
    if mode == 'bf16':
        return (v32.view(torch.int32) & ~0xffff).view(torch.float32).double()
    near = v32.to(torch.float16)
    bits = near.view(torch.int16)
    # (the pattern of a magnitude one step smaller, whatever the sign)
    bits = torch.where(near.float().abs() > v32.abs(), bits - 1, bits)
    return bits.view(torch.float16).double()


def tie_margin(v64, mode):
    """Smallest relative distance of the non-zero values of `v64` from a
    rounding tie of the 16-bit type (inf for an empty tensor)."""
    v64 = v64[v64 != 0]
    if v64.numel() == 0:
        return float('inf')
    near = v64.float().to(HALF[mode]).double()
    mant, exp = torch.frexp(near)
    above = torch.exp2(exp.double() - PRECISION[mode])   # grid above |near|
    below = torch.where(mant.abs() == .5, above / 2, above)
    d = v64.abs() - near.abs()
    half = torch.where(d >= 0, above, below) / 2
    return ((half - d.abs()) / v64.abs()).min().item()


def edge_rows(frames):
    t = torch.arange(frames)
    return (t < 3) | (t >= frames - 3)


# ---------------------------------------------------------------------------
# ConvNeXt block
# ---------------------------------------------------------------------------
def layer_norm(x, p, mode):
    """The depthwise conv and the LayerNorm of the block: (the operand xn
    (B, T, 512) float64, |v rstd g|, the tie margin)."""
    c = x.shape[-1]
    frames = x.shape[1]
    g, beta = p['norm.weight'].double(), p['norm.bias'].double()
    v = F.conv1d(x.double().transpose(1, 2), p['dwconv.weight'].double(),
                 None, padding=3, groups=c).transpose(1, 2)
    if not (((v == 0) | (v.abs() == 8)).all() and not v.sum(-1).any()):
        raise NotExact('the conv outputs are not balanced +-8 / 0')
    var = (v * v).sum(-1, keepdim=True) / c             # n / 8: exact in fp32
    var32 = (var.float() + _EPS).double()               # the fp32 addition
    if not torch.equal(var32[:, 3:frames - 3], var[:, 3:frames - 3]):
        raise NotExact('an interior variance is not 64')
    scaled = v * var32.rsqrt() * g
    xn64 = scaled + beta
    if not ((xn64 == 0) | (xn64.abs() >= .5)).all():
        raise NotExact('an xn below 0.5')
    if mode == 'fp32':
        return xn64, scaled.abs(), float('inf')
    margin = tie_margin(xn64, mode)
    if not margin >= TIE_MARGIN:
        raise NotExact(f'an xn {margin:.2e} from a rounding tie')
    return cvt(xn64.float(), mode), scaled.abs(), margin


def block(x, p, mode):
    """x (B, T, 512) fp32 channels-last, p the block's fp32 tensors (state
    dict leaves). Returns a dict: want (B, T, 512) float64, bits, margin and,
    for fp32, bound (the per-element error bound)."""
    assert mode in MODES and not p['dwconv.bias'].any()
    frames = x.shape[1]
    b1, b2 = p['pwconv1.bias'].double(), p['pwconv2.bias'].double()
    gamma = p['gamma'].double()
    w1 = cvt(p['pwconv1.weight'], mode)
    w2 = cvt(p['pwconv2.weight'], mode)
    edge = edge_rows(frames).double()[None, :, None]
    xn, scaled, margin = layer_norm(x, p, mode)

    c1 = xn @ w1.T
    bound1 = xn.abs() @ w1.abs().T
    v1 = c1 + b1
    if not (v1.abs() >= 16).all():
        raise NotExact('a pre-activation inside +-16')
    h64 = v1.clamp(min=0)
    h = h64 if mode == 'fp32' else cvt(h64.float(), mode)
    c2 = h @ w2.T
    bound2 = h.abs() @ w2.abs().T
    y = x.double() + gamma * (c2 + b2)

    out = dict(want=y, margin=margin, bits=0., xn=xn, v1=v1, h=h)
    if mode != 'fp32':
        if mode == 'f16' and max(xn.abs().max(), v1.abs().max()) >= E.F16_MAX:
            raise NotExact('an operand beyond the f16 range')
        if not torch.equal(v1.float().double(), v1):
            raise NotExact('c1 + b1 does not fit fp32')
        q2 = quantum(h) * quantum(w2)
        out['bits'] = max(
            exactness(c1, bound1.max().item(), quantum(xn) * quantum(w1)),
            exactness(c2, bound2.max().item(), q2),
            exactness(y, (x.double().abs() + gamma * (bound2 + b2.abs()))
                      .max().item(),
                      min(quantum(x.double()),
                          quantum(gamma) * min(q2, quantum(b2)))))
        return out

    # fp32: RSTD_ERROR in rstd on every row; on edge rows one rounding each
    # for v rstd, (.) g, (.) + beta, every non-zero term of a contraction,
    # + b1, + b2 and x + (.). gelu (|v| >= 16) and gamma (2**k) round nothing.
    nnz1 = (w1 != 0).sum(1).max().item()
    nnz2 = (w2 != 0).sum(1).max().item()
    e_xn = RSTD_ERROR * scaled + edge * U * (2 * scaled + xn.abs())
    e_v = e_xn @ w1.abs().T + edge * U * (nnz1 * bound1 + v1.abs())
    if not (v1.abs() - e_v >= 15.5).all():
        raise NotExact('a pre-activation may leave the saturated GELU')
    e_h = e_v * (v1 > 0)
    e_acc = e_h @ w2.abs().T + edge * U * (nnz2 * bound2 + (c2 + b2).abs())
    out['bound'] = gamma * e_acc + edge * U * y.abs()
    return out


def emulate_block(x, p, mode, defect=None):
    """vocos_block_kernel step by step in fp32 on the CPU, for the planted
    defects of test_cpu_vocos_exact.py (defect None: the kernel as written).
    (B, T, 512) fp32 out."""
    assert defect in (None, 'truncate xn', 'truncate h', 'b1 after rounding',
                      'tap off by one', 'halo across utterances',
                      'chunk skipped', 'chunk without hc', 'gamma before b2')
    batch, frames, c = x.shape
    rows = batch * frames
    hidden = p['pwconv1.weight'].shape[0]
    flat = x.reshape(rows, c)
    r = torch.arange(rows)
    t = r % frames
    dw = p['dwconv.weight'][:, 0].T                     # [7][C]
    s = torch.zeros(rows, c)
    for tap in range(7):
        off = tap - 3
        ok = (t + off >= 0) & (t + off < frames)
        if defect == 'halo across utterances':
            ok = (r + off >= 0) & (r + off < rows)
        src = off + (1 if defect == 'tap off by one' else 0)
        rows_in = flat[(r + src).clamp(0, rows - 1)]
        s = torch.where(ok[:, None], rows_in * dw[tap] + s, s)
    v = s + p['dwconv.bias']
    v = v - (v.sum(-1, keepdim=True) * (1. / c))
    var = (v * v).sum(-1, keepdim=True) * (1. / c)
    rstd = 1. / torch.sqrt(var + _EPS)
    xn = cvt(v * rstd * p['norm.weight'] + p['norm.bias'], mode,
             defect == 'truncate xn')
    w1 = cvt(p['pwconv1.weight'], mode)
    w2 = cvt(p['pwconv2.weight'], mode)
    acc = torch.zeros(rows, c)
    for hc in range(0, hidden, CHUNK):
        if defect == 'chunk skipped' and hc == hidden - CHUNK:
            continue
        # (exact on these inputs whatever the order: the oracle asserts it)
        c1 = (xn @ w1[hc:hc + CHUNK].T).float()
        bias = p['pwconv1.bias'][hc:hc + CHUNK]
        if defect == 'b1 after rounding':
            c1 = cvt(c1, mode).float()
        u = c1 + bias
        gelu = .5 * u * (1. + torch.erf(u * 0.70710678118654752440))
        h = cvt(gelu, mode, defect == 'truncate h')
        at = 0 if defect == 'chunk without hc' else hc
        acc = acc + (h @ w2[:, at:at + CHUNK].T).float()
    if defect == 'gamma before b2':
        y = flat + (p['gamma'] * acc + p['pwconv2.bias'])
    else:
        y = flat + p['gamma'] * (acc + p['pwconv2.bias'])
    return y.view(batch, frames, c)


# --- the case table --------------------------------------------------------
BLOCK_HIDDEN = (64, 192, 1536)
# (B, T): every row an edge row (T <= 3: taps outside on both sides); 133
# rows - a tile boundary of the MT = 128 and of the MT = 64 template inside
# utterances, many utterance ends in one tile; 390 rows - a partial last tile
BLOCK_SHAPES = ((2, 1), (1, 5), (4, 6), (19, 7), (3, 130))
# channels of the tap classes 0 .. 6 (even; the centre tap, the only live one
# at T = 1, is the largest: 8 sqrt(8 / n) stays in [1.05, 1.52] on edge rows)
TAP_CLASSES = (48, 48, 48, 224, 48, 48, 48)
BIG_G = 515.        # bf16 holds multiples of 4 there; 515 + {0, +-2} is odd
BIG_B1 = 2048.      # f16 holds even integers beyond, bf16 multiples of 16
NNZ = 8             # non-zeros of a row of W1 and of W2


_choice = E._choice


def block_weights(hidden, seed):
    """The block's tensors but pwconv1.bias, which needs the rounded xn."""
    c = CHANNELS
    gen = torch.Generator().manual_seed(seed)
    order = torch.randperm(c, generator=gen)
    tau = torch.empty(c, dtype=torch.int64)
    tau[order] = torch.repeat_interleave(
        torch.arange(7), torch.tensor(TAP_CLASSES))
    sign = _choice((-1, 1), (c,), gen)
    dw = torch.zeros(c, 1, 7)
    dw[torch.arange(c), 0, tau] = sign
    # g odd, beta even; |g| 1 with beta 0 / +-4 and |g| 3 with 0 / +-2 keep
    # every edge-row xn at least 0.5 from zero (asserted by block())
    size = _choice((1, 3), (c,), gen)
    g = size * _choice((-1, 1), (c,), gen)
    beta = _choice((-1, 0, 1), (c,), gen) * torch.where(size == 1, 4., 2.)
    # W1: row h holds channels cols[8 h .. 8 h + 7] of a permutation, +-1
    cols = torch.randperm(c, generator=gen)
    w1 = torch.zeros(hidden, c)
    w2 = torch.zeros(c, hidden)
    units = torch.randperm(hidden, generator=gen)
    for j in range(NNZ):
        w1[torch.arange(hidden), cols[(NNZ * torch.arange(hidden) + j) % c]] = \
            _choice((-1, 1), (hidden,), gen)
        w2[torch.arange(c), units[(NNZ * torch.arange(c) + j) % hidden]] = \
            _choice((-1, 1), (c,), gen)
    # four channels that bf16 cannot hold, each in a W1 row of its own
    big = cols[torch.arange(4) * NNZ]
    g[big] = BIG_G * _choice((-1, 1), (4,), gen)
    beta[big] = torch.tensor([0., 2., -2., 0.])
    return {'dwconv.weight': dw, 'dwconv.bias': torch.zeros(c),
            'norm.weight': g, 'norm.bias': beta, 'pwconv1.weight': w1,
            'pwconv2.weight': w2,
            'pwconv2.bias': _choice(range(-9, 10), (c,), gen),
            'gamma': _choice((.5, 1., 2.), (c,), gen)}, tau, sign


def block_input(batch, frames, tau, sign, seed):
    """x = 8 s sign(w), s = +-1 balanced within every tap class of every row"""
    gen = torch.Generator().manual_seed(seed)
    s = torch.empty(batch, frames, CHANNELS)
    for tap, n in enumerate(TAP_CLASSES):
        half = torch.cat([torch.ones(n // 2), -torch.ones(n // 2)])
        order = torch.rand(batch, frames, n, generator=gen).argsort(-1)
        s[:, :, tau == tap] = half[order]
    return 8 * s * sign


def pre_activation_bias(x, p, mode, seed):
    """b1[h] = +-(16 + bound of row h's contraction (+ BIG_B1 every 16th
    unit)); one unit in four is negative (a dead unit: h = 0 on every row)."""
    xn, _, _ = layer_norm(x, p, mode)
    bound = (xn.abs() @ p['pwconv1.weight'].double().abs().T)
    bound = bound.flatten(0, 1).max(0).values.ceil()
    hidden = bound.numel()
    gen = torch.Generator().manual_seed(seed)
    size = 16 + bound + _choice((0, 1), (hidden,), gen).double()
    size[5::16] += BIG_B1
    sign = torch.where(torch.arange(hidden) % 4 == 3, -1., 1.).double()
    return (sign * size).float()


@functools.lru_cache(maxsize=None)
def block_case(mode, hidden, batch, frames):
    seed = 10000 * hidden + 100 * batch + frames
    p, tau, sign = block_weights(hidden, hidden)
    x = block_input(batch, frames, tau, sign, seed)
    p['pwconv1.bias'] = pre_activation_bias(x, p, mode, seed + 1)
    out = block(x, p, mode)
    out.update(x=x, p=p, tau=tau)
    return out


# ---------------------------------------------------------------------------
# vocos_gemm_kernel
# ---------------------------------------------------------------------------
def gemm(x, w, bias, gbias, mode, channels_first):
    """conv1d ('same', zero padding at every utterance's ends) of the cvt of
    x ((B, K, T) when channels_first, else (B, T, K)) and w (N, K, taps),
    + bias + gbias[b] (gbias (1 | B, N) or None; both fp32 in the epilogue):
    ((B, T, N) float64, bits)."""
    a = cvt(x if channels_first else x.transpose(1, 2).contiguous(), mode)
    wr = cvt(w, mode)
    if mode == 'f16' and max(a.abs().max(), wr.abs().max()) >= E.F16_MAX:
        raise NotExact('an operand beyond the f16 range')
    every = bias.double()[None, :, None].expand(a.shape[0], -1, -1)
    if gbias is not None:
        every = every + gbias.double()[:, :, None]
    pad = w.shape[-1] // 2
    y = F.conv1d(a, wr, None, padding=pad) + every
    bound = F.conv1d(a.abs(), wr.abs(), None, padding=pad) + every.abs()
    q = min(quantum(a) * quantum(wr), quantum(every))
    return y.transpose(1, 2), exactness(y, bound.max().item(), q)


def emulate_gemm(x, w, bias, gbias, mode, channels_first, defect=None):
    """vocos_gemm_kernel's result in fp32 with a planted defect."""
    assert defect in (None, 'last column block dropped',
                      'gbias of the wrong utterance')
    if defect == 'gbias of the wrong utterance' and gbias.shape[0] > 1:
        gbias = gbias.roll(1, 0)
    y, _ = gemm(x, w, bias, gbias, mode, channels_first)
    y = y.float()
    if defect == 'last column block dropped':
        y[:, :, (w.shape[0] - 1) // 128 * 128:] = 0
    return y


# name: taps, channels_first, K, N, gbias
GEMM_KERNELS = {'conv_pre': (7, True, 80, 512, True),
                'embed': (7, False, 512, 512, False),
                'head': (1, False, 512, 1026, False)}
# rows 1, 31, 33, 100 and 130
GEMM_SHAPES = ((1, 1), (1, 31), (3, 11), (20, 5), (2, 65))
# operands the 16-bit types cannot hold, ties among them (257, 2049: exactly
# known inputs round deterministically)
GEMM_LARGE = (257., 259., -261., 515., 2049., -2051., 4099.)


def gemm_table():
    """(name, gbatch) of every contraction case: gbatch 0 - no gbias."""
    return [('conv_pre', 1), ('conv_pre', 'B'), ('embed', 0), ('head', 0)]


@functools.lru_cache(maxsize=None)
def gemm_case(mode, name, gbatch, batch, frames):
    taps, cf, k, n, _ = GEMM_KERNELS[name]
    gen = torch.Generator().manual_seed(1000 * k + 10 * batch + frames)
    w = _choice(range(-2, 3), (n, k, taps), gen)
    bias = _choice(range(-99, 100), (n,), gen)
    x = _choice(range(-64, 65), (batch, k, frames) if cf else
                (batch, frames, k), gen)
    count = min(4 * len(GEMM_LARGE), x.numel() // 2)
    at = torch.randperm(x.numel(), generator=gen)[:count]
    x.view(-1)[at] = torch.tensor(GEMM_LARGE * 4)[:count]
    gbias = None
    if gbatch:
        gbias = _choice(range(-999, 1000),
                        (batch if gbatch == 'B' else 1, n), gen)
    y, bits = gemm(x, w, bias, gbias, mode, cf)
    return dict(x=x, w=w, bias=bias, gbias=gbias, want=y, bits=bits,
                taps=taps, cf=cf)
