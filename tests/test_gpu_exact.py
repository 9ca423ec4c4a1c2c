"""The conv kernels against a float64 oracle with `torch.equal`: no tolerance.

The inputs (exact_oracle.py) are small integers chosen so that every product
and every partial sum of a conv is exactly representable in fp32; the result
then does not depend on the order of summation, and a wrong index, tap,
column, channel, dilation, rounding mode or stale byte shows as whole units of
the value grid. test_gpu_kernels.py keeps guarding what these inputs cannot:
conditioning on realistic values, DENSE weights over three fused iterations
and the ledger of measured errors.

One iteration runs dense, two sparse (two weights 10 {+-1} per row), three -
what every production Block has - lifted: the sparse construction continued
to three reaches 24.8 - 25.1 bits in bf16 and leaves the f16 range, because
it multiplies by 10 at every conv; a lifted Block does so in one iteration
only, the signed one, and keeps the hidden activations of the other two
non-negative with a constant bias (exact_oracle.py: 14.0 - 16.6 bits, the
largest operand 53 240 < 65504, in all five modes).

Every case asserts its exactness (<= 22 bits of bound / q, the result a
fixed point of a round trip through fp32) before it compares; the case table
is checked on the CPU by test_cpu_exact_oracle.py.

Kernel forms reached (the form is part of a Block test's id, and every Block
and MRF launch is held to it through pm_debug_last_launch: the library's own
report of the kernel and the segments it took, not E.block_form's restatement
of the planner):
  test_block_iteration           conv_pair_kernel (C >= 128: latency geometry)
  test_block_iteration_wide_tiles  conv_pair_kernel, wide geometry, C 128 / 256
  test_whole_block[...-tiled]    conv_block3_kernel (two-sided tiling)
  test_whole_block[...-walked]   conv_block3_walk_kernel, 2 and 3 segments
  test_whole_block[...-skewed]   conv_block3_skew_kernel, 2 and 3 segments
                                 (each with n1, n2 and n3 iterations)
  test_block_output_as_operand   conv_block3_skew_kernel's 16-bit hand-over
  test_whole_mrf                 conv_mrf_kernel, the two-sided whole-MRF
                                 tiling: all there is for one and two
                                 iterations (plan_mrf_cfg) - the hooks are set
                                 as for the others all the same
  test_whole_mrf_three_iterations[...-tiled]   conv_mrf_kernel
  test_whole_mrf_three_iterations[...-walked]  conv_mrf_walk_kernel, 16-bit
                                 operands, 2 and 3 segments
  test_whole_mrf_three_iterations[...-skewed]  conv_mrf_skew_kernel, 4-byte
                                 operands, 1, 2 and 3 segments
  test_conv_transpose            conv_single_kernel, conv_upsample_kernel with
                                 1, 2 and all M groups; the 16-bit input path
  test_conv_transpose_long_batch conv_single_kernel, 256 input columns a
                                 workgroup (long batches), 128 one utterance
                                 below the threshold
  test_input_conv                conv_single_kernel with the speaker bias
"""
import ctypes

import pytest
import torch

import exact_oracle as E
from util import from_cl, pad32, to_cl

pytestmark = pytest.mark.gpu

HALF = {'f16': torch.float16, 'bf16': torch.bfloat16}


def lib():
    from promonet_amd import _lib
    return _lib


def assert_exact(case):
    assert case['bits'] <= E.EXACT_BITS, case['bits']


def assert_equal(got, want, detail):
    got = got.double().cpu()
    assert torch.equal(got, want), (detail, E.first_difference(got, want))


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# PmKernel of pm_launch.h
KERNELS = {1: 'skewed', 2: 'walked', 3: 'tiled'}


def last_launch():
    """(form, segments, act16) of this thread's last pm_block_cl /
    pm_block_act16_cl / pm_mrf_cl, from the library (pm_debug_last_launch)."""
    _lib = lib()
    kernel, nseg, narrow, act16 = (ctypes.c_int(-1) for _ in range(4))
    _lib.check(_lib.lib().pm_debug_last_launch(
        *[ctypes.byref(v) for v in (kernel, nseg, narrow, act16)]))
    return KERNELS[kernel.value], nseg.value, bool(act16.value)


def assert_launch(form, nseg, act16=False):
    """The device ran what the test's id says: E.block_form restates the
    planner, this is the planner's own answer. A two-sided tiling has no
    segments."""
    assert last_launch() == (form, nseg if form != 'tiled' else 0, act16)


# ---------------------------------------------------------------------------
# (a) one iteration, dense; (f) the f16 operand edge
# ---------------------------------------------------------------------------
def run_iteration(device, mode, x, w, k, d, store_mode=0, scale=1., prev=None):
    _lib = lib()
    b, c, length = x.shape
    x_cl = to_cl(x).to(device)
    out = torch.zeros_like(x_cl) if prev is None else to_cl(prev).to(device)
    size = _lib.lib().pm_op_workspace_bytes(c, c, k)
    ws = torch.empty(size, dtype=torch.uint8, device=device)
    tensors = [t.to(device).contiguous() for t in w]
    _lib.check(_lib.lib().pm_block_iteration_cl(
        _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out),
        *[_lib.ptr(t) for t in tensors], b, length, c, k, d, store_mode, scale,
        ws.data_ptr(), ws.numel(), _lib.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('channels', E.ITERATION_CHANNELS)
@pytest.mark.parametrize('kernel_size', E.ITERATION_KERNELS)
def test_block_iteration(device, mode, channels, kernel_size):
    for d, length, store_mode in E.ITERATION_RUNS:
        case = E.iteration_case(mode, channels, kernel_size, d, length, store_mode)
        assert_exact(case)
        out = run_iteration(
            device, mode, case['x'], case['w'], kernel_size, d, store_mode,
            E.SCALES[store_mode], case['prev'])     # (`out` pre-filled)
        assert_equal(from_cl(out, channels), case['want'],
                     (d, length, store_mode))
        # padded output channels stay exactly zero
        padded = out[:, :, channels:]
        assert padded.numel() == 0 or not padded.any()


@pytest.mark.parametrize('mode', ['f16', 'bf16'])
@pytest.mark.parametrize('channels', [c for c, _, _ in E.ITERATION_WIDE])
def test_block_iteration_wide_tiles(device, mode, channels):
    """The pair kernel's wide geometry at C = 128 / 256 (the lengths above
    all take the latency geometry): 152 workgroups, a ragged last tile."""
    case = E.iteration_wide_case(mode, channels)
    assert_exact(case)
    out = run_iteration(device, mode, case['x'], case['w'], 3, 3, 2,
                        E.SCALES[2], case['prev'])
    assert_equal(from_cl(out, channels), case['want'], channels)


@pytest.mark.parametrize('mode', ['f16', 'f16x3', 'f16a2'])
def test_f16_operand_edge(device, mode):
    """Activations at 65504, on both sides of the last rounding boundary
    below it (65488), around the boundary to infinity (65520) and far above,
    in conv1 and - two saturated operands summed - in conv2: bit for bit the
    oracle, which has the clamp."""
    case = E.f16_edge_case(mode)
    assert_exact(case)
    out = run_iteration(device, mode, case['x'], case['w'], case['k'], case['d'])
    assert_equal(from_cl(out, 32), case['want'], mode)


# ---------------------------------------------------------------------------
# (b), (c) whole-Block kernels
# ---------------------------------------------------------------------------
class BlockRunner:
    """pm_block_cl / pm_block_act16_cl on a Block case in one of the forms
    the launcher has for the shape, through the test hooks."""

    def __init__(self, device, mode, c, k, request, form=None):
        _lib = lib()
        self.device, self.mode, self.c, self.k = device, mode, c, k
        self.request = request
        # the kernel the test's id names: the library's report is held to it
        self.form = form or E.block_form(mode, c, k, request)
        self.weights = 3 * _lib.lib().pm_op_workspace_bytes(c, c, k)
        scratch = _lib.lib().pm_walk_scratch_bytes(E.BATCH)
        assert scratch > 0
        self.ws = torch.empty(
            self.weights + (scratch if request == 'skewed' else 0),
            dtype=torch.uint8, device=device)

    def __call__(self, case, act=None):
        _lib = lib()
        x_cl = to_cl(case['x']).to(self.device)
        out = to_cl(case['prev']).to(self.device)
        w = [[t.to(self.device).contiguous() for t in ts] for ts in case['w']]
        dil = (ctypes.c_int * len(case['dilations']))(*case['dilations'])
        forced = self.request != 'own'
        _lib.check(_lib.lib().pm_debug_force(case['nseg'] if forced else 0, 0))
        _lib.check(_lib.lib().pm_debug_skew(
            {'own': 0, 'walked': -1, 'skewed': 1}[self.request]))
        if self.request == 'skewed':
            self.ws[self.weights:].fill_(0xff)  # (NaNs: nothing stale is read)
        args = [*[pointers(ts) for ts in w], dil, len(case['dilations']),
                E.BATCH, case['length'], self.c, self.k, case['store_mode'],
                E.SCALES[case['store_mode']], self.ws.data_ptr(),
                self.ws.numel(), _lib.stream()]
        act16 = None
        if act is None:
            _lib.check(_lib.lib().pm_block_cl(
                _lib.DTYPES[self.mode], _lib.ptr(x_cl), _lib.ptr(out), *args))
        else:
            act16 = torch.full(
                (E.BATCH, case['length'], pad32(self.c)), 0x7fff,
                dtype=torch.int16, device=self.device)
            _lib.check(_lib.lib().pm_block_act16_cl(
                _lib.DTYPES[self.mode], _lib.DTYPES[act], _lib.ptr(x_cl),
                _lib.ptr(out), act16.data_ptr(), *args))
        torch.cuda.synchronize()
        assert_launch(self.form, case['nseg'], act is not None)
        return out, act16


def restore_hooks():
    _lib = lib()
    _lib.check(_lib.lib().pm_debug_force(0, 0))
    _lib.check(_lib.lib().pm_debug_skew(0))


BLOCK_CASES = [
    pytest.param(mode, c, k, niter, request, id='-'.join((
        mode, f'C{c}', f'k{k}', f'n{niter}', E.block_form(mode, c, k, request))))
    for mode, c, k, niter in E.block_table()
    for request in E.block_requests(mode, c, k)]


@pytest.mark.parametrize('mode,channels,kernel_size,niter,request_', BLOCK_CASES)
def test_whole_block(device, mode, channels, kernel_size, niter, request_):
    """niter = 1: dense, each of d = 1, 3, 5. niter = 2: sparse, the pairs
    (1, 3), (3, 5), (5, 1) - the hand-over of the trunk between iterations
    (the 32 i skew, the carries through LDS and scratch). niter = 3: lifted
    (exact_oracle.py), the rotations of (1, 3, 5) - what production
    launches: the third iteration, the 64-column skew, the second hand-over,
    the 60-column halo at k 11. 2 and 3 segments, uneven, a boundary that is
    no tile multiple, an utterance end inside a tile, L = 61 and
    2 columns + 1; every store mode. The library says which kernel ran
    (BlockRunner)."""
    run = BlockRunner(device, mode, channels, kernel_size, request_)
    try:
        for index in range(3):
            case = E.block_case(mode, channels, kernel_size, niter, index)
            assert_exact(case)
            out, _ = run(case)
            assert_equal(from_cl(out, channels), case['want'],
                         (case['nseg'], case['length'], case['dilations']))
    finally:
        restore_hooks()


def test_form_assertion_is_live(device):
    """pm_debug_last_launch follows the launch, not the request's name: the
    same case on the skewed walk, then as the launcher chooses - whose
    report fails the skewed id's assertion - and a thread that has launched
    nothing is told so."""
    import threading
    mode, c, k = 'bf16', 64, 7
    case = E.block_case(mode, c, k, 3, 1)
    try:
        BlockRunner(device, mode, c, k, 'skewed')(case)
        assert last_launch() == ('skewed', case['nseg'], False)
        BlockRunner(device, mode, c, k, 'own')(case)
        assert last_launch() == ('tiled', 0, False)
        with pytest.raises(AssertionError):
            BlockRunner(device, mode, c, k, 'own', form='skewed')(case)
        seen = []
        worker = threading.Thread(target=lambda: seen.append(
            lib().lib().pm_debug_last_launch(
                *[ctypes.byref(ctypes.c_int()) for _ in range(4)])))
        worker.start()
        worker.join()
        assert seen == [lib().PM_ESTATE]
    finally:
        restore_hooks()


@pytest.mark.parametrize('act', ['f16', 'bf16'])
@pytest.mark.parametrize('mode', ['f16', 'bf16'])
@pytest.mark.parametrize('channels,kernel_size,niter',
                         [(128, 11, 1), (64, 7, 2), (128, 11, 3), (64, 7, 3)])
def test_block_output_as_operand(device, mode, act, channels, kernel_size, niter):
    """pm_block_act16_cl on Block cases: act16 holds the oracle's operand
    bits, cvt(lrelu(result)) in the next stage's type, `out` is left alone."""
    run = BlockRunner(device, mode, channels, kernel_size, 'skewed')
    try:
        for index in (0, 1):
            case = E.block_case(mode, channels, kernel_size, niter, index)
            assert_exact(case)
            out, act16 = run(case, act)
            assert torch.equal(out.cpu(), to_cl(case['prev']))
            operand = E.round_operand(
                E.lrelu32(case['want'].float()), act, 'act')
            want = to_cl(operand).to(HALF[act]).view(torch.int16)
            assert torch.equal(act16[:, :, :channels].cpu(),
                               want[:, :, :channels]), (index, act)
    finally:
        restore_hooks()


# ---------------------------------------------------------------------------
# (d) the whole MRF
# ---------------------------------------------------------------------------
class MrfRunner:
    """pm_mrf_cl on the MRF cases of (mode, channels, niter): the workspace
    holds the packed weights and, behind them, the skewed walk's scratch,
    which a launch is handed or not."""

    def __init__(self, device, mode, channels, niter):
        _lib = lib()
        self.device, self.mode, self.channels = device, mode, channels
        self.niter = niter
        per = _lib.lib().pm_op_workspace_bytes(channels, channels, 11)
        self.weights = 3 * niter * per
        scratch = _lib.lib().pm_walk_scratch_bytes(E.BATCH)
        assert scratch > 0
        self.ws = torch.empty(
            self.weights + scratch, dtype=torch.uint8, device=device)

    def __call__(self, case, nseg, scratch, form):
        """The launch forced to `nseg` segments (0: the launcher's choice),
        with or without scratch; asserts the kernel the library reports and
        the derived bound; returns `out` as the kernel left it."""
        _lib = lib()
        x_cl = to_cl(case['x']).to(self.device)
        order = [[t.to(self.device).contiguous()
                  for block in case['blocks'] for t in block[which]]
                 for which in range(4)]
        dil = (ctypes.c_int * self.niter)(*case['dilations'])
        _lib.check(_lib.lib().pm_debug_force(nseg, 0))
        self.ws[self.weights:].fill_(0xff)  # (NaNs: nothing stale is read)
        out = torch.full_like(x_cl, 7.)
        _lib.check(_lib.lib().pm_mrf_cl(
            _lib.DTYPES[self.mode], _lib.ptr(x_cl), _lib.ptr(out),
            *[pointers(ts) for ts in order], dil, self.niter, E.BATCH,
            case['length'], self.channels, self.ws.data_ptr(),
            self.ws.numel() if scratch else self.weights, _lib.stream()))
        torch.cuda.synchronize()
        assert_launch(form, nseg)
        bound = 4 * 2. ** -24 * sum(p.abs() for p in case['parts']) / 3
        got = from_cl(out, self.channels).double().cpu()
        error = (got - case['total'] / 3).abs()
        assert (error <= bound).all(), (
            form, nseg, case['length'], (error - bound).max().item(),
            E.first_difference(got, case['total'] / 3))
        return out


@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('channels', E.MRF_CHANNELS)
@pytest.mark.parametrize('niter', [1, 2])
def test_whole_mrf(device, mode, channels, niter):
    """The sum S of the three Blocks is exact; the final * (1 / 3) is one or
    more fp32 roundings of partial results (at most three: each Block's share
    or the sum's), and whether they are fused is the compiler's, so
    |got - S / 3| <= 4 * 2**-24 * (|B3| + |B7| + |B11|) / 3 elementwise -
    derived, not measured. One and two iterations have the two-sided tiling
    only, whatever the hooks ask for (asserted)."""
    run = MrfRunner(device, mode, channels, niter)
    wide = mode not in ('f16', 'bf16')
    try:
        for index in range(len(E.MRF_LENGTHS)):
            case = E.mrf_case(mode, channels, niter, index)
            assert_exact(case)
            run(case, 0, False, 'tiled')
            run(case, 2, wide, 'tiled')
    finally:
        restore_hooks()


# The whole-MRF kernels of three iterations (plan_mrf_cfg): (form, segments
# forced, scratch handed over)
MRF_FORMS = {'tiled': ((0, False),),
             'walked': ((2, False), (3, False)),
             'skewed': ((1, True), (2, True), (3, True))}


def mrf_forms(mode):
    return ('tiled', 'walked') if mode in HALF else ('tiled', 'skewed')


@pytest.mark.parametrize('mode,channels,form', [
    pytest.param(mode, c, form, id=f'{mode}-C{c}-n3-{form}')
    for mode in E.MODES for c in E.MRF_CHANNELS for form in mrf_forms(mode)])
def test_whole_mrf_three_iterations(device, mode, channels, form):
    """What production launches: three lifted Blocks (exact_oracle.py) of
    three iterations each, the rotations of (1, 3, 5). conv_mrf_kernel (no
    force, no scratch), conv_mrf_walk_kernel (16-bit operands, 2 and 3
    segments), conv_mrf_skew_kernel (4-byte operands, 1, 2 and 3 segments,
    scratch behind the weights - NaNs before every launch); L = 1, 61,
    2 NC + 1 and 5 NC + 37 of the k 11 geometry's NC columns. Held to the
    bound of test_whole_mrf, and the walked and the skewed launch bit for bit
    to the two-sided tiling, whose sum order (B11 + B7 + B3) / 3 is theirs
    (test_gpu_kernels.py::test_whole_mrf)."""
    run = MrfRunner(device, mode, channels, 3)
    try:
        for index in range(len(E.MRF_LENGTHS)):
            case = E.mrf_case(mode, channels, 3, index)
            assert_exact(case)
            tiled = run(case, 0, False, 'tiled')
            if form == 'tiled':
                continue
            for nseg, scratch in MRF_FORMS[form]:
                out = run(case, nseg, scratch, form)
                assert torch.equal(out, tiled), (nseg, case['length'])
    finally:
        restore_hooks()


# ---------------------------------------------------------------------------
# (e) the upsamplers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('c_in,c_out,rate', E.UPSAMPLE_SHAPES)
def test_conv_transpose(device, mode, c_in, c_out, rate):
    _lib = lib()
    half = mode in HALF
    wide = half and rate == 8 and c_in >= 256
    size = _lib.lib().pm_op_workspace_bytes(c_in, c_out, 2 * rate)
    ws = torch.empty(size, dtype=torch.uint8, device=device)
    try:
        for length in E.UPSAMPLE_LENGTHS:
            case = E.upsample_case(mode, c_in, c_out, rate, length)
            assert_exact(case)
            x_cl = to_cl(case['x']).to(device)
            wd, bd = case['w'].to(device), case['bias'].to(device)
            for groups in ((0, 1, 2) if wide else (0,)):
                _lib.check(_lib.lib().pm_debug_force(0, groups))
                out = torch.full((E.BATCH, length * rate, pad32(c_out)), 7.,
                                 device=device)
                _lib.check(_lib.lib().pm_conv_transpose_cl(
                    _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out),
                    _lib.ptr(wd), _lib.ptr(bd), E.BATCH, length, c_in, c_out,
                    rate, 1, ws.data_ptr(), ws.numel(), _lib.stream()))
                torch.cuda.synchronize()
                assert_equal(from_cl(out, c_out), case['want'],
                             (length, groups))
            if half and not wide:
                # the input already staged as 16-bit operands
                _lib.check(_lib.lib().pm_debug_force(0, 0))
                operand = E.round_operand(E.lrelu32(case['x']), mode, 'act')
                staged, bits = E.conv_transpose(
                    operand.float(), case['w'], case['bias'], mode, rate,
                    staged=True)
                assert bits <= E.EXACT_BITS
                assert torch.equal(staged, case['want'])
                x16 = to_cl(operand).to(HALF[mode]).to(device)
                out = torch.full((E.BATCH, length * rate, pad32(c_out)), 7.,
                                 device=device)
                _lib.check(_lib.lib().pm_conv_transpose_x16_cl(
                    _lib.DTYPES[mode], x16.data_ptr(), _lib.ptr(out),
                    _lib.ptr(wd), _lib.ptr(bd), E.BATCH, length, c_in, c_out,
                    rate, ws.data_ptr(), ws.numel(), _lib.stream()))
                torch.cuda.synchronize()
                assert_equal(from_cl(out, c_out), staged, (length, 'x16'))
    finally:
        restore_hooks()


@pytest.mark.parametrize(
    'mode,batch,length,drawn',
    [(mode, *run) for mode in HALF for run in E.UPSAMPLE_LONG])
def test_conv_transpose_long_batch(device, mode, batch, length, drawn):
    """The 256-column variant of the C_in 128 r = 2 upsampler, and at batch
    511 the 128-column one on the same data (E.UPSAMPLE_LONG)"""
    _lib = lib()
    c_in, c_out, rate = 128, 64, 2
    case = E.upsample_long_case(mode, length, drawn)
    assert_exact(case)
    x_cl = to_cl(case['x'][:batch]).to(device)
    wd, bd = case['w'].to(device), case['bias'].to(device)
    size = _lib.lib().pm_op_workspace_bytes(c_in, c_out, 2 * rate)
    ws = torch.empty(size, dtype=torch.uint8, device=device)
    out = torch.full((batch, length * rate, c_out), float('nan'),
                     device=device)
    _lib.check(_lib.lib().pm_conv_transpose_cl(
        _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out), _lib.ptr(wd),
        _lib.ptr(bd), batch, length, c_in, c_out, rate, 1, ws.data_ptr(),
        ws.numel(), _lib.stream()))
    torch.cuda.synchronize()
    assert_equal(from_cl(out, c_out), case['want'][:batch], (batch, length))


# ---------------------------------------------------------------------------
# (g) the input conv with its speaker conv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', E.INPUT_MODES)
@pytest.mark.parametrize('shape', E.INPUT_SHAPES)
def test_input_conv(device, mode, shape):
    _lib = lib()
    c_in, c_out, G = shape
    for index, (batch, length, gbatch) in enumerate(E.INPUT_RUNS):
        case = E.input_case(mode, c_in, c_out, G, index)
        assert_exact(case)
        on_device = [case[name].to(device).contiguous()
                     for name in ('w', 'bias', 'sw', 'sb')]
        x_cl = to_cl(case['x']).to(device)
        glob = case['g'].to(device).contiguous()
        out = torch.full((batch, length, pad32(c_out)), 7., device=device)
        size = _lib.lib().pm_op_workspace_bytes(c_in, c_out, 7) + \
            256 * ((batch * pad32(c_out) * 4 + 255) // 256)
        ws = torch.empty(size, dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().pm_input_conv_cl(
            _lib.DTYPES[mode], _lib.ptr(x_cl), _lib.ptr(out),
            *[_lib.ptr(t) for t in on_device[:2]], _lib.ptr(glob),
            *[_lib.ptr(t) for t in on_device[2:]], gbatch, G, batch, length,
            c_in, c_out, ws.data_ptr(), ws.numel(), _lib.stream()))
        torch.cuda.synchronize()
        assert_equal(from_cl(out, c_out), case['want'], (batch, length, gbatch))
