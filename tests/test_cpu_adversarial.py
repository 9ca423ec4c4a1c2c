"""The adversarial losses of promonet_amd.loss without a GPU: the oracle
(tests/adversarial_oracle.py) against the golden from the reference and
against autograd, the ABI table and its argument checks, the checks of the
Python entry points, and the cap of the Gaussian gate of
tests/test_gpu_adversarial.py."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib

import adversarial_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ('pm_multi_mean_chunk', 'pm_multi_mean_workspace_bytes',
           'pm_multi_mean', 'pm_multi_mean_backward')
FLAGS = [(hinge, omit) for hinge in (False, True) for omit in (False, True)]


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'adversarial.pt')


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('hinge,omit_first', FLAGS)
def test_oracle_equals_the_reference_golden(golden, hinge, omit_first):
    """The golden's sums are exact in fp32 (powers of two of elements on a
    dyadic grid): float64 must equal the reference's fp32 run to the bit."""
    maps, logits = golden['maps'], golden['logits']
    want = golden['results'][f'hinge{int(hinge)}/omit{int(omit_first)}']

    def exact(got, name):
        assert got.dtype == torch.float64
        assert torch.equal(got, want[name].double()), name

    exact(oracle.feature_matching(maps['real'], maps['fake'], omit_first),
          'feature_matching')
    total, real_losses, fake_losses = oracle.discriminator(
        logits['real'], logits['fake'], hinge)
    exact(total, 'discriminator')
    exact(torch.stack(real_losses), 'discriminator_real')
    exact(torch.stack(fake_losses), 'discriminator_fake')
    total, losses = oracle.generator(logits['fake'], hinge)
    exact(total, 'generator')
    exact(torch.stack(losses), 'generator_losses')


def test_golden_inputs_hold_the_edge_cases(golden):
    maps, logits = golden['maps'], golden['logits']
    assert sum(len(m) for m in maps['real']) + \
        sum(len(m) for m in maps['fake']) == 12
    for reals, fakes in zip(maps['real'], maps['fake']):
        for real, fake in zip(reals, fakes):
            assert real.numel() <= 1200 and (real == fake).any()
            assert (real != fake).any()
    for side in ('real', 'fake'):
        for tensor in logits[side]:
            assert (tensor == 1).any() and (tensor == -1).any()
    # the shape lists the benchmark scales: 5 period, 3 resolution, 1
    # multi-band discriminators of 30, 18 and 26 maps
    shapes = golden['shapes']
    assert [len(shapes[name]) for name in
            ('period', 'resolution', 'multiband')] == [5, 3, 1]
    assert sum(len(maps) for maps in shapes['period']) == 30
    assert sum(len(maps) for maps in shapes['resolution']) == 18
    assert sum(len(maps) for maps in shapes['multiband']) == 26
    assert golden['batch_size'] == 64 and golden['chunk_size'] == 16384


def edge_logits(seed):
    """float64 logits with values exactly at +1 and -1"""
    tensors = [oracle.gaussian((3, 17), seed).double(),
               oracle.gaussian((2, 5, 7), seed + 1).double()]
    for tensor in tensors:
        tensor.flatten()[:4] = torch.tensor([1., -1., 1., -1.])
    return tensors


@pytest.mark.parametrize('hinge,omit_first', FLAGS)
def test_oracle_gradients_equal_autograd(hinge, omit_first):
    real_maps = [[oracle.gaussian((2, 3, 5), 1).double(),
                  oracle.gaussian((2, 4, 3, 2), 2).double()],
                 [oracle.gaussian((1, 7), 3).double(),
                  oracle.gaussian((2, 2), 4).double()]]
    fake_maps = [[oracle.gaussian(m.shape, 10 + i + 2 * j).double()
                  for j, m in enumerate(maps)]
                 for i, maps in enumerate(real_maps)]
    for reals, fakes in zip(real_maps, fake_maps):
        for real, fake in zip(reals, fakes):
            fake.flatten()[::3] = real.flatten()[::3]       # equal elements
    leaves = [[f.clone().requires_grad_(True) for f in fakes]
              for fakes in fake_maps]
    # the reference's formula through autograd
    loss = 0.
    for reals, fakes in zip(real_maps, leaves):
        for real, fake in list(zip(reals, fakes))[int(omit_first):]:
            loss = loss + torch.mean(torch.abs(real - fake))
    loss.backward()
    want = oracle.feature_matching_gradient(real_maps, fake_maps, omit_first)
    for fakes, gradients in zip(leaves, want):
        for index, (fake, gradient) in enumerate(zip(fakes, gradients)):
            if omit_first and index == 0:
                assert fake.grad is None and not gradient.any()
            else:
                assert torch.equal(fake.grad, gradient)
                assert (gradient == 0).any()
    assert torch.equal(
        oracle.feature_matching(real_maps, fake_maps, omit_first),
        loss.detach())

    reals = [t.requires_grad_(True) for t in edge_logits(20)]
    fakes = [t.requires_grad_(True) for t in edge_logits(30)]
    if hinge:
        loss = sum(torch.mean(torch.clamp(1. - r, min=0.)) for r in reals) + \
            sum(torch.mean(torch.clamp(1 + f, min=0.)) for f in fakes)
    else:
        loss = sum(torch.mean((1. - r) ** 2.) for r in reals) + \
            sum(torch.mean(f ** 2.) for f in fakes)
    loss.backward()
    detached = [[t.detach() for t in side] for side in (reals, fakes)]
    want = oracle.discriminator_gradient(*detached, hinge)
    for side, gradients in zip((reals, fakes), want):
        for leaf, gradient in zip(side, gradients):
            assert torch.allclose(leaf.grad, gradient, rtol=1e-15, atol=0)
    if hinge:
        # the boundary passes the gradient: -1 / numel at +1, +1 / numel at -1
        assert want[0][0].flatten()[0] == -1. / 51
        assert want[1][0].flatten()[1] == 1. / 51

    outputs = [t.requires_grad_(True) for t in edge_logits(40)]
    if hinge:
        loss = sum(torch.mean(torch.clamp(1. - o, min=0.)) for o in outputs)
    else:
        loss = sum(torch.mean((1. - o) ** 2.) for o in outputs)
    loss.backward()
    want = oracle.generator_gradient([o.detach() for o in outputs], hinge)
    for leaf, gradient in zip(outputs, want):
        assert torch.allclose(leaf.grad, gradient, rtol=1e-15, atol=0)


@pytest.mark.parametrize('op', oracle.OPS)
def test_fp32_gradient_restatement_follows_the_float64_gradient(op):
    """One division and at most one rounding product: within 3 x 2^-24"""
    a = oracle.gaussian((5, 41), 50 + op)
    b = oracle.gaussian((5, 41), 60 + op)
    a.flatten()[:2] = torch.tensor([1., -1.])
    b.flatten()[2:4] = a.flatten()[2:4]
    for g in (1., 3.):
        got = oracle.gradient_fp32(op, a, b, g).double()
        want = g * oracle.derivative(op, a.double(), b.double()) / a.numel()
        assert ((got - want).abs() <= 3 * 2. ** -24 * want.abs()).all()
        assert torch.equal(got == 0, want == 0)


###############################################################################
# The ABI
###############################################################################


def test_the_constants_agree():
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    for name in ('ABS_DIFF', 'SQ_ONE_MINUS', 'SQ', 'HINGE_ONE_MINUS',
                 'HINGE_ONE_PLUS'):
        value = int(re.search(
            rf'#define PM_ADV_{name} (\d+)', header).group(1))
        assert value == getattr(_lib, f'ADV_{name}') == getattr(oracle, name)
    assert promonet_amd.ADVERSARIAL_HINGE_LOSS is False
    assert promonet_amd.FEATURE_MATCHING_OMIT_FIRST is False
    try:
        promonet_amd.configure(
            ADVERSARIAL_HINGE_LOSS=True, FEATURE_MATCHING_OMIT_FIRST=True)
        assert promonet_amd.config.ADVERSARIAL_HINGE_LOSS is True
        assert promonet_amd.FEATURE_MATCHING_OMIT_FIRST is True
    finally:
        promonet_amd.configure(
            ADVERSARIAL_HINGE_LOSS=False, FEATURE_MATCHING_OMIT_FIRST=False)


def test_abi_entries_and_their_argument_checks():
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    declared = set(re.findall(r'\b(pm_[a-z0-9_]+)\s*\(', header))
    library = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in declared, name
        assert hasattr(library, name), name
    chunk = library.pm_multi_mean_chunk()
    assert chunk > 0 and chunk % (oracle.THREADS * oracle.VEC) == 0

    def longs(*values):
        return (ctypes.c_longlong * len(values))(*values)

    def ints(*values):
        return (ctypes.c_int * len(values))(*values)

    def pointers(*values):
        return (ctypes.c_void_p * len(values))(*values)

    # the workspace: per entry 16 + 8 bytes and one float a chunk, each part
    # rounded to 256 bytes; 0 for a bad list
    size = library.pm_multi_mean_workspace_bytes
    assert size(longs(1, chunk, chunk + 1), 3) == 3 * 256
    assert size(longs(*([1] * 17)), 17) == 512 + 256 + 256
    assert size(longs(65 * chunk), 1) == 256 + 256 + 512
    assert size(None, 1) == 0
    assert size(longs(5), 0) == 0
    assert size(longs(5, 0), 2) == 0
    assert size(longs(-1), 1) == 0

    # every bad argument answers -1 before any device work (the pointers are
    # made up and never followed)
    fake = 0x1000
    good = dict(a=pointers(fake), b=pointers(fake), numel=longs(5),
                op=ints(0), dtype=ints(0), count=1, out=fake,
                workspace=fake, size=1 << 20)

    def forward(**changes):
        v = dict(good, **changes)
        return library.pm_multi_mean(
            v['a'], v['b'], v['numel'], v['op'], v['dtype'], v['count'],
            v['out'], v['workspace'], v['size'], None)

    def backward(**changes):
        v = dict(dict(good, grad_out=fake, grad_a=None,
                      grad_b=pointers(fake)), **changes)
        return library.pm_multi_mean_backward(
            v['a'], v['b'], v['numel'], v['op'], v['dtype'], v['count'],
            v['grad_out'], v['grad_a'], v['grad_b'], None, 0, None)

    bad = (dict(count=0), dict(count=-3), dict(a=None), dict(numel=None),
           dict(op=None), dict(dtype=None), dict(b=None),
           dict(numel=longs(0)), dict(numel=longs(-7)), dict(op=ints(5)),
           dict(op=ints(-1)), dict(dtype=ints(3)), dict(dtype=ints(-1)),
           dict(a=pointers(None)), dict(b=pointers(None)))
    for changes in bad:
        assert forward(**changes) == -1, changes
        assert library.pm_last_error()
        assert backward(**changes) == -1, changes
    assert forward(out=None) == -1
    assert forward(workspace=None) == -1
    assert forward(size=3 * 256 - 1) == -1
    assert b'workspace' in library.pm_last_error()
    assert backward(grad_out=None) == -1
    assert backward(grad_a=None, grad_b=None) == -1
    # the real maps are constants: no gradient for a of ABS_DIFF
    assert backward(grad_a=pointers(fake)) == -1
    assert b'PM_ADV_ABS_DIFF' in library.pm_last_error()
    # b is not read by the logit ops: the array may be missing
    assert forward(op=ints(1), b=None, size=0) == -1
    assert b'workspace' in library.pm_last_error()


###############################################################################
# The Python entry points (they answer before any device is touched)
###############################################################################


def test_value_errors_come_before_any_device_work():
    loss = promonet_amd.loss
    maps = [[torch.zeros(2, 3, 4), torch.zeros(2, 5)], [torch.zeros(1, 7)]]
    same = [[torch.zeros_like(m) for m in group] for group in maps]
    with pytest.raises(ValueError, match='lists'):
        loss.feature_matching(maps, same[:1])
    with pytest.raises(ValueError, match='2 real maps and 1 fake maps'):
        loss.feature_matching(maps, [same[0][:1], same[1]])
    with pytest.raises(ValueError, match='differ in shape'):
        loss.feature_matching(maps, [[same[0][0], torch.zeros(2, 6)], same[1]])
    with pytest.raises(ValueError, match='is empty'):
        loss.feature_matching(
            [[torch.zeros(2, 0)]], [[torch.zeros(2, 0)]])
    with pytest.raises(ValueError, match='no feature maps'):
        loss.feature_matching([], [])
    with pytest.raises(ValueError, match='no feature maps'):
        loss.feature_matching([[]], [[]])
    with pytest.raises(ValueError, match='float tensor'):
        loss.feature_matching([[torch.zeros(3, dtype=torch.int32)]],
                              [[torch.zeros(3, dtype=torch.int32)]])
    try:
        promonet_amd.configure(FEATURE_MATCHING_OMIT_FIRST=True)
        # nothing is left once the first maps are gone
        with pytest.raises(ValueError, match='no feature maps'):
            loss.feature_matching([maps[1]], [same[1]])
    finally:
        promonet_amd.configure(FEATURE_MATCHING_OMIT_FIRST=False)

    logits = [torch.zeros(2, 9), torch.zeros(2, 4)]
    with pytest.raises(ValueError, match='2 entries, fake_outputs 1'):
        loss.discriminator(logits, logits[:1])
    with pytest.raises(ValueError, match='differ in shape'):
        loss.discriminator(logits, logits[::-1])
    with pytest.raises(ValueError, match='is empty'):
        loss.discriminator([], [])
    with pytest.raises(ValueError, match=r'real_outputs\[1\] is empty'):
        loss.discriminator([logits[0], torch.zeros(0)],
                           [logits[0], torch.zeros(0)])
    with pytest.raises(ValueError, match='is empty'):
        loss.generator([])
    with pytest.raises(ValueError, match=r'discriminator_outputs\[0\] is empty'):
        loss.generator([torch.zeros(3, 0)])
    # ... and there is no CPU fallback behind the checks
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss.feature_matching(maps, same)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss.discriminator(logits, logits)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss.generator(logits)


###############################################################################
# The conditions of tests/test_gpu_adversarial.py
###############################################################################


def test_the_gaussian_gate_stays_within_four_times_the_fp32_restatement():
    """K of the Gaussian test is 3x the figure measured on an MI355X and may
    not exceed 4x the figure of the fp32 CPU restatement with the kernel's
    chunked order on the same inputs."""
    import test_gpu_adversarial as gpu
    chunk = _lib.lib().pm_multi_mean_chunk()
    worst = max(gpu.restatement_figure(dtype, chunk) for dtype in gpu.DTYPES)
    gate, measured = gpu.GAUSSIAN_GATE
    print(f'gate {gate}, measured {measured}, fp32 CPU {worst:.4g}')
    assert gate <= 4 * worst
    assert measured < gate <= 3.001 * measured


def test_the_exact_inputs_keep_every_sum_exact():
    """Every sum of terms over the grid unit stays below 2^24, so fp32 adds
    them exactly in any order (asserted again, from the same inputs, on the
    GPU)"""
    import test_gpu_adversarial as gpu
    chunk = _lib.lib().pm_multi_mean_chunk()
    for dtype in gpu.DTYPES:
        entries = gpu.exact_entries(chunk, dtype)
        assert len(entries) == 35
        gpu.assert_sums_are_exact(entries)
