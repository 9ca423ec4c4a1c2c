"""The adversarial losses on the GPU against tests/adversarial_oracle.py:
the multi-tensor mean kernels (pm_adv.h) through `_MultiMean`, and
`feature_matching`, `discriminator` and `generator` through autograd.

Exact tests: inputs on a dyadic grid that fp32, f16 and bf16 all hold and on
which every sum is exact in fp32 (asserted from the inputs), so means and
total must be `torch.equal` to the float64 oracle rounded once, and the
gradients to the fp32 restatement of the backward (oracle.gradient_fp32).

Gaussian test: the model is a relative 2^-24 on each mean (and the total).
The gate is K x the model; K = 3 x the largest figure measured on an MI355X
(GAUSSIAN_GATE lists the measurement) and at most 4 x the figure of the fp32
CPU restatement with the kernel's chunked order (oracle.chunked_mean) on the
same inputs, which tests/test_cpu_adversarial.py asserts. The device's means
are also held to that restatement bit for bit.
"""
import functools
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib

import adversarial_oracle as oracle
from util import check

ROOT = Path(__file__).resolve().parent.parent
EPS = 2. ** -24
UNIT = 2. ** -4             # every term of the exact inputs is a multiple
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
DTYPE_IDS = ('fp32', 'f16', 'bf16')
# (K, the largest figure measured on the MI355X): K = 3 x measured. Per dtype
# the device measured 2.2843 (fp32), 2.0474 (f16) and 2.6573 (bf16); the fp32
# CPU restatement reaches the same three figures on the same inputs, because
# its means are the device's bit for bit (asserted below), so the cap of 4 x
# the restatement, 10.63, does not bind
GAUSSIAN_GATE = (7.97, 2.6573)


def sizes(chunk):
    """(numel, storage offset): one element, less than a wave, around one
    chunk, several chunks with a tail, and a view that is not 16-byte
    aligned"""
    return ((1, 0), (63, 0), (chunk - 1, 0), (chunk, 0), (chunk + 1, 0),
            (3 * chunk + 5, 0), (chunk + 3, 1))


###############################################################################
# Inputs (CPU tensors; computed once a dtype and left unchanged)
###############################################################################


@functools.lru_cache(maxsize=None)
def exact_entries(chunk, dtype):
    """Every size with every op: multiples of 2^-4 in [-2, 2] for ABS_DIFF
    with equal pairs, multiples of 2^-2 in [-2, 2] with +1 and -1 for the
    logit ops"""
    entries, seed = [], 100
    for numel, offset in sizes(chunk):
        for op in oracle.OPS:
            seed += 2
            if op == oracle.ABS_DIFF:
                a = oracle.grid((numel,), 2. ** -4, seed, dtype)
                b = oracle.grid((numel,), 2. ** -4, seed + 1, dtype)
                b[::5] = a[::5]
            else:
                a = oracle.grid((numel,), 2. ** -2, seed, dtype)
                a[:2] = torch.tensor([1., -1.], dtype=dtype)[:numel]
                b = None
            entries.append({'op': op, 'a': a, 'b': b, 'offset': offset})
    return tuple(entries)


@functools.lru_cache(maxsize=None)
def gaussian_entries(chunk, dtype):
    entries, seed = [], 300
    for numel, offset in sizes(chunk):
        for op in oracle.OPS:
            seed += 2
            entries.append({
                'op': op, 'a': oracle.gaussian((numel,), seed, dtype),
                'b': oracle.gaussian((numel,), seed + 1, dtype)
                if op == oracle.ABS_DIFF else None, 'offset': offset})
    return tuple(entries)


def assert_sums_are_exact(entries):
    """From the inputs: every term is a multiple of 2^-4 and the sum of a
    tensor's terms over 2^-4 stays below 2^24, so every partial sum is an
    fp32 number whatever the order"""
    for e in entries:
        a = e['a'].double()
        assert torch.equal(a, e['a'].float().double())
        terms = oracle.term(
            e['op'], a, None if e['b'] is None else e['b'].double()) / UNIT
        assert torch.equal(terms, terms.round())
        assert terms.sum().item() < 2. ** 24, (e['op'], a.numel())


def ops_of(entries):
    return tuple(e['op'] for e in entries)


@functools.lru_cache(maxsize=None)
def truth(kind, chunk, dtype):
    """(means, total) of the float64 oracle, once a case"""
    entries = (exact_entries if kind == 'exact' else gaussian_entries)(
        chunk, dtype)
    return oracle.multi_mean(
        ops_of(entries), [e['a'] for e in entries], [e['b'] for e in entries])


def figure(means, total, want):
    """The largest error of a mean or the total in units of 2^-24 relative"""
    got = torch.cat([means.double(), total.double().reshape(1)])
    want = torch.cat([want[0], want[1].reshape(1)])
    return ((got - want).abs() / want.abs() / EPS).max().item()


@functools.lru_cache(maxsize=None)
def restatement(dtype, chunk):
    """(means, total) of the fp32 CPU restatement in the kernel's order"""
    means = [oracle.chunked_mean(e['op'], e['a'], e['b'], chunk)
             for e in gaussian_entries(chunk, dtype)]
    total = torch.zeros((), dtype=torch.float64)
    for mean in means:
        total = total + mean
    return torch.stack(means).float(), total.float()


def restatement_figure(dtype, chunk):
    return figure(*restatement(dtype, chunk), truth('gaussian', chunk, dtype))


###############################################################################
# Through the kernels
###############################################################################


def on_device(tensor, device, offset=0):
    """A copy on the device that starts `offset` elements into its storage"""
    storage = torch.empty(
        tensor.numel() + offset, dtype=tensor.dtype, device=device)
    view = storage[offset:].view(tensor.shape)
    view.copy_(tensor)
    assert view.storage_offset() == offset
    return view


def run(device, entries, g=None):
    """(means, total) on the CPU and, with g, the gradients of g * total: of
    b for ABS_DIFF, of a for the other ops"""
    count = len(entries)
    ops = ops_of(entries)
    a = [on_device(e['a'], device, e['offset']) for e in entries]
    # (b is not read by the logit ops: any tensor of the size does)
    b = [a[k].detach() if e['b'] is None else on_device(e['b'], device)
         for k, e in enumerate(entries)]
    leaves = [b[k] if op == oracle.ABS_DIFF else a[k]
              for k, op in enumerate(ops)]
    if g is not None:
        for leaf in leaves:
            leaf.requires_grad_(True)
    total, means = promonet_amd.loss._MultiMean.apply(ops, count, *a, *b)
    assert not means.requires_grad
    if g is None:
        return means.cpu(), total.cpu()
    (g * total).backward()
    return means.detach().cpu(), total.detach().cpu(), \
        [leaf.grad.cpu() for leaf in leaves]


def want_gradients(entries, g):
    return [oracle.gradient_fp32(e['op'], e['a'], e['b'], g) for e in entries]


def assert_exact(device, entries, want):
    assert_sums_are_exact(entries)
    for g in (1., 3.):
        means, total, gradients = run(device, entries, g)
        assert means.dtype == total.dtype == torch.float32
        assert torch.equal(means, want[0].float())
        assert torch.equal(total, want[1].float())
        for e, got, expected in zip(
                entries, gradients, want_gradients(entries, g)):
            assert got.dtype == e['a'].dtype
            assert torch.equal(got, expected), (e['op'], e['a'].numel(), g)


@pytest.fixture(scope='module')
def chunk():
    return _lib.lib().pm_multi_mean_chunk()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_exact_values_and_gradients(device, chunk, dtype):
    entries = exact_entries(chunk, dtype)
    assert len(entries) == 35
    for e in entries:
        if e['op'] == oracle.ABS_DIFF:
            assert (e['a'] == e['b']).any()
        elif e['a'].numel() > 1:
            assert (e['a'] == 1).any() and (e['a'] == -1).any()
    assert_exact(device, entries, truth('exact', chunk, dtype))


@pytest.mark.gpu
def test_a_list_longer_than_one_launch(device):
    """70 tensors of 1 to 70 elements: two launches over one partials buffer;
    the ops and the dtypes go round"""
    entries = []
    for k in range(70):
        op, dtype = oracle.OPS[k % 5], DTYPES[k % 3]
        step = 2. ** -4 if op == oracle.ABS_DIFF else 2. ** -2
        entries.append({
            'op': op, 'a': oracle.grid((k + 1,), step, 500 + 2 * k, dtype),
            'b': oracle.grid((k + 1,), step, 501 + 2 * k, dtype)
            if op == oracle.ABS_DIFF else None, 'offset': 0})
    want = oracle.multi_mean(
        ops_of(entries), [e['a'] for e in entries], [e['b'] for e in entries])
    assert_exact(device, entries, want)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_gaussian_inputs(device, chunk, dtype):
    entries = gaussian_entries(chunk, dtype)
    want = truth('gaussian', chunk, dtype)
    means, total, gradients = run(device, entries, 1.)
    measured = figure(means, total, want)
    restated = restatement(dtype, chunk)
    print(f'gaussian {dtype}: {measured:.4f} x 2^-24 (fp32 CPU restatement '
          f'{restatement_figure(dtype, chunk):.4f}; the same bits: '
          f'{torch.equal(means, restated[0])}, '
          f'{torch.equal(total, restated[1])})')
    check(measured, GAUSSIAN_GATE[0], 'adversarial/gaussian', dtype)
    # pm_adv.o is built without contraction: the restatement is the kernel's
    # arithmetic operation for operation
    assert torch.equal(means, restated[0])
    assert torch.equal(total, restated[1])
    # the gradient is elementwise: the restatement's bits
    for e, got, expected in zip(
            entries, gradients, want_gradients(entries, 1.)):
        assert torch.equal(got, expected), (e['op'], e['a'].numel())


@pytest.mark.gpu
def test_runs_are_bit_identical_and_a_mean_does_not_depend_on_its_list(
        device, chunk):
    entries = gaussian_entries(chunk, torch.float32)
    first = run(device, entries, 1.)
    second = run(device, entries, 1.)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])
    for one, other in zip(first[2], second[2]):
        assert torch.equal(one, other)
    for dtype in DTYPES:
        entries = gaussian_entries(chunk, dtype)
        means, _ = run(device, entries)
        for k, e in enumerate(entries):
            alone, total = run(device, [e])
            assert torch.equal(alone[0], means[k]), (dtype, k)
            assert torch.equal(total, alone[0])
            # ... nor on its alignment
            moved = dict(e, offset=1 - e['offset'])
            assert torch.equal(run(device, [moved])[0][0], means[k])


###############################################################################
# Through the module
###############################################################################


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'adversarial.pt')


@pytest.fixture
def flags(request):
    hinge, omit_first = request.param
    promonet_amd.configure(
        ADVERSARIAL_HINGE_LOSS=hinge, FEATURE_MATCHING_OMIT_FIRST=omit_first)
    yield hinge, omit_first
    promonet_amd.configure(
        ADVERSARIAL_HINGE_LOSS=False, FEATURE_MATCHING_OMIT_FIRST=False)


def leaves(tensors, device, dtype=None):
    return [t.to(device, dtype).requires_grad_(True) for t in tensors]


def assert_gradients(got, inputs, op, want, fake=None, g=1.):
    """Every gradient against the fp32 restatement, to the bit, and against
    the float64 gradient of the oracle"""
    for index, (leaf, a, gradient) in enumerate(zip(got, inputs, want)):
        b = None if fake is None else fake[index]
        assert leaf.grad.dtype == leaf.dtype
        assert leaf.grad.shape == leaf.shape
        assert torch.equal(
            leaf.grad.cpu(), oracle.gradient_fp32(op, a, b, g))
        assert ((leaf.grad.cpu().double() - g * gradient).abs()
                <= 3 * EPS * g * gradient.abs()).all()


@pytest.mark.gpu
@pytest.mark.parametrize(
    'flags', [(h, o) for h in (False, True) for o in (False, True)],
    indirect=True)
def test_the_three_losses_equal_the_golden(device, golden, flags):
    """The golden's values are exact in fp32 (the reference's own run, which
    the float64 oracle equals to the bit: test_cpu_adversarial.py)"""
    hinge, omit_first = flags
    maps, logits = golden['maps'], golden['logits']
    want = golden['results'][f'hinge{int(hinge)}/omit{int(omit_first)}']
    loss = promonet_amd.loss

    real = [leaves(m, device) for m in maps['real']]
    fake = [leaves(m, device) for m in maps['fake']]
    value = loss.feature_matching(real, fake)
    assert value.ndim == 0 and value.dtype == torch.float32
    assert torch.equal(value.cpu(), want['feature_matching'])
    (3. * value).backward()
    gradients = oracle.feature_matching_gradient(
        maps['real'], maps['fake'], omit_first)
    for d in range(len(real)):
        # the real maps are constants
        assert all(leaf.grad is None for leaf in real[d])
        skip = int(omit_first)
        assert all(leaf.grad is None for leaf in fake[d][:skip])
        assert_gradients(
            fake[d][skip:], maps['real'][d][skip:], oracle.ABS_DIFF,
            gradients[d][skip:], maps['fake'][d][skip:], 3.)

    real, fake = leaves(logits['real'], device), leaves(logits['fake'], device)
    total, real_losses, fake_losses = loss.discriminator(real, fake)
    assert torch.equal(total.cpu(), want['discriminator'])
    assert torch.equal(torch.stack(real_losses).cpu(),
                       want['discriminator_real'])
    assert torch.equal(torch.stack(fake_losses).cpu(),
                       want['discriminator_fake'])
    # the per-discriminator losses are for logging
    assert total.requires_grad
    assert not any(l.requires_grad for l in real_losses + fake_losses)
    total.backward()
    ops = oracle.logit_ops(1, hinge, True)
    gradients = oracle.discriminator_gradient(
        logits['real'], logits['fake'], hinge)
    assert_gradients(real, logits['real'], ops[0], gradients[0])
    assert_gradients(fake, logits['fake'], ops[1], gradients[1])

    outputs = leaves(logits['fake'], device)
    total, losses = loss.generator(outputs)
    assert torch.equal(total.cpu(), want['generator'])
    assert torch.equal(torch.stack(losses).cpu(), want['generator_losses'])
    assert not any(l.requires_grad for l in losses)
    total.backward()
    assert_gradients(outputs, logits['fake'], ops[0],
                     oracle.generator_gradient(logits['fake'], hinge))


@pytest.mark.gpu
def test_memory_formats_and_views_equal_their_contiguous_copies(device):
    """Inputs on the grid, so that the order of a sum does not matter: a
    channels-last pair is read as it lies, a view that is not dense is
    copied, and both give the bits of the contiguous copies"""
    loss = promonet_amd.loss
    real = oracle.grid((2, 6, 5, 7), 2. ** -4, 700).to(device)
    fake = oracle.grid((2, 6, 5, 7), 2. ** -4, 701).to(device)
    wide = oracle.grid((2, 6, 5, 14), 2. ** -4, 702).to(device)

    def both(real, fake):
        leaf = fake.detach().requires_grad_(True)
        value = loss.feature_matching([[real]], [[leaf]])
        value.backward()
        return value.detach(), leaf.grad

    want = both(real, fake)
    last = both(real.contiguous(memory_format=torch.channels_last),
                fake.contiguous(memory_format=torch.channels_last))
    assert torch.equal(last[0], want[0]) and torch.equal(last[1], want[1])
    assert last[1].is_contiguous(memory_format=torch.channels_last)
    # one side channels-last, the other contiguous
    mixed = both(real.contiguous(memory_format=torch.channels_last), fake)
    assert torch.equal(mixed[0], want[0]) and torch.equal(mixed[1], want[1])
    # every other column of a wider map: not dense
    view = wide[..., ::2]
    assert not view.is_contiguous()
    want = both(real, view.contiguous())
    got = both(real, view)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    logit = view[:, 0].detach().requires_grad_(True)
    copy = view[:, 0].contiguous().requires_grad_(True)
    loss.generator([logit])[0].backward()
    loss.generator([copy])[0].backward()
    assert torch.equal(logit.grad, copy.grad)


@pytest.mark.gpu
def test_bf16_maps_return_bf16_gradients(device, golden):
    maps, logits = golden['maps'], golden['logits']
    loss = promonet_amd.loss
    real = [leaves(m, device, torch.bfloat16) for m in maps['real']]
    fake = [leaves(m, device, torch.bfloat16) for m in maps['fake']]
    value = loss.feature_matching(real, fake)
    assert value.dtype == torch.float32
    # (the grid is exact in bf16: the fp32 run's value)
    assert torch.equal(
        value.cpu(), golden['results']['hinge0/omit0']['feature_matching'])
    value.backward()
    for fakes, reals, cpu in zip(fake, maps['real'], maps['fake']):
        for leaf, a, b in zip(fakes, reals, cpu):
            assert leaf.grad.dtype == torch.bfloat16
            assert torch.equal(leaf.grad.cpu(), oracle.gradient_fp32(
                oracle.ABS_DIFF, a.bfloat16(), b.bfloat16()))
    outputs = leaves(logits['fake'], device, torch.bfloat16)
    loss.generator(outputs)[0].backward()
    assert all(o.grad.dtype == torch.bfloat16 for o in outputs)
    # a pair of two dtypes is read as fp32; each gradient in its leaf's dtype
    half = leaves(maps['fake'][0][:1], device, torch.float16)
    loss.feature_matching([[real[0][0]]], [half]).backward()
    assert half[0].grad.dtype == torch.float16


@pytest.mark.gpu
def test_forward_and_backward_capture_into_one_graph(device, golden):
    maps, logits = golden['maps'], golden['logits']
    loss = promonet_amd.loss
    real_maps = [[m.to(device) for m in group] for group in maps['real']]
    fake_maps = [leaves(m, device) for m in maps['fake']]
    real, fake = [t.to(device).requires_grad_(True) for t in logits['real']], \
        leaves(logits['fake'], device)
    inputs = [m for group in fake_maps for m in group] + real + fake

    def step():
        value = loss.feature_matching(real_maps, fake_maps) + \
            loss.discriminator(real, fake)[0] + 2. * loss.generator(fake)[0]
        return value, torch.autograd.grad(value, inputs)

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        value, gradients = step()
    with torch.no_grad():
        for index, tensor in enumerate(inputs):
            tensor.copy_(oracle.gaussian(tensor.shape, 900 + index))
    graph.replay()
    torch.cuda.synchronize(device)
    replayed = value.clone(), [g.clone() for g in gradients]
    eager = step()
    assert torch.equal(replayed[0], eager[0])
    for one, other in zip(replayed[1], eager[1]):
        assert torch.equal(one, other)
