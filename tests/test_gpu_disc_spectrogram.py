"""promonet_amd.model.discriminator on the GPU against the float64 oracle
(tests/disc_spectrogram_oracle.py): forward and gradient of the three
spectrograms, and the properties of each mode.

Every gate is K x an error model of an fp32 transform (delta = 2^-24 log2(N)
|windowed frame|_2 per frame):
  forward R / CMB   delta per bin;
  forward DB        (20 / ln 10) delta / |X|;
  grad_x            2^-24 log2 N, relative L2 per row;
K = 4 x the largest figure that the reference's own arithmetic in fp32
(torch.stft and the torch ops of the three methods, on the CPU) shows on the
same inputs, per family (oracle.GATES; test_cpu_disc_spectrogram.py holds
them to the recorded figures). The fragile bins are left out of the forward
comparison and carry no upstream gradient. Each test prints its figure beside
the fp32 CPU one; DESIGN section 19 lists both.
"""
import types

import pytest
import torch

import promonet_amd
from promonet_amd import _lib
from promonet_amd.model import discriminator

import disc_spectrogram_oracle as oracle
from util import check

NAMES = list(oracle.CASES)
MAGNITUDE = [name for name in NAMES if oracle.family(name) == 'magnitude']
DECIBEL = [name for name in NAMES if oracle.family(name) == 'DB']


def run(name, x):
    """The public function of a case as ONE tensor (CMB: the bands side by
    side, which is the tensor they are views of)"""
    kind, sizes, _ = oracle.CASES[name]
    if kind == 'R':
        return discriminator.spectrogram_resolution(x, sizes)
    if kind == 'DB':
        return discriminator.spectrogram_decibel(x, sizes)
    assert (promonet_amd.WINDOW_SIZE, promonet_amd.HOPSIZE) == sizes[:2]
    return torch.cat(discriminator.spectrogram_multiband(x), -1)


def forward_backward(device, name, x=None, upstream=None):
    want = oracle.truth(name)
    leaf = (want['x'] if x is None else x).to(device).requires_grad_(True)
    out = run(name, leaf)
    upstream = want['upstream'] if upstream is None else upstream
    out.backward(upstream.to(device).reshape(out.shape))
    return out.detach(), leaf.grad


###############################################################################
# Against the oracle
###############################################################################


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_forward(device, name):
    want = oracle.truth(name)
    out = run(name, want['x'].to(device))
    assert out.shape == want['out'].shape and out.dtype == torch.float32
    figure = oracle.figure_forward(name, out.cpu())
    print(f'forward {name}: {figure:.3f} x the model '
          f'(fp32 CPU {oracle.fp32_figures(name)[0]:.3f}, gate '
          f'{oracle.gate(name, "forward"):.3f})')
    check(figure, oracle.gate(name, 'forward'), 'disc_spec/forward', name)
    if oracle.family(name) == 'DB':
        # the floored elements are the oracle's, and they show one value
        floored = want['out'] == want['out'].min()
        keep = ~want['fragile']
        assert torch.equal((out.cpu() == out.min().cpu())[keep], floored[keep])
        assert floored[1].any() and not floored[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_gradient(device, name):
    want = oracle.truth(name)
    _, gradient = forward_backward(device, name)
    assert gradient.shape == want['x'].shape
    figure = oracle.figure_gradient(name, gradient.cpu())
    print(f'gradient {name}: {figure:.3f} x 2^-24 log2 N '
          f'(fp32 CPU {oracle.fp32_figures(name)[1]:.3f}, gate '
          f'{oracle.gate(name, "gradient"):.3f})')
    check(figure, oracle.gate(name, 'gradient'), 'disc_spec/gradient', name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_gradient_accumulates_into_what_is_there(device, name):
    """The backward entry with accumulate: grad_x += the same bits, in one
    fp32 add, scaled by a device scalar"""
    kind, sizes, _ = oracle.CASES[name]
    want = oracle.truth(name)
    flat = want['x'].to(device)
    checked = discriminator._sizes(
        {'R': _lib.DISC_SPEC_R, 'CMB': _lib.DISC_SPEC_CMB,
         'DB': _lib.DISC_SPEC_DB}[kind], sizes, flat.shape[1])
    tables = discriminator._tables(device, checked)
    out, stats = discriminator._forward_call(flat, *tables, checked)
    upstream = want['upstream'].to(device).reshape(out.shape).contiguous()
    saved = (out, stats) if kind == 'DB' else ()
    plain = discriminator._backward_call(
        flat, *tables, checked, upstream, *saved)
    _, through_autograd = forward_backward(device, name)
    assert torch.equal(plain, through_autograd)
    into = want['start'].to(device)
    summed = discriminator._backward_call(
        flat, *tables, checked, upstream, *saved, into=into.clone())
    assert torch.equal(summed, into + plain)
    figure = oracle.figure_gradient(
        name, (summed - into).cpu(), want['gradient'])
    scale = torch.full((1,), -.5, device=device)
    scaled = discriminator._backward_call(
        flat, *tables, checked, upstream, *saved, into=into.clone(),
        scale=scale)
    assert torch.equal(scaled, into + -.5 * plain)
    # (summed - into rounds once more, at the size of `into`: no gate on it)
    print(f'accumulate {name}: {figure:.3f} x 2^-24 log2 N after the '
          'subtraction')


###############################################################################
# R and CMB
###############################################################################


@pytest.mark.gpu
@pytest.mark.parametrize('name', MAGNITUDE)
def test_zero_input_gives_exact_zeros(device, name):
    want = oracle.truth(name)
    out, gradient = forward_backward(
        device, name, x=torch.zeros_like(want['x']))
    assert torch.equal(out, torch.zeros_like(out))
    assert torch.equal(gradient, torch.zeros_like(gradient))


@pytest.mark.gpu
@pytest.mark.parametrize('name', MAGNITUDE)
def test_a_row_does_not_depend_on_its_batch(device, name):
    want = oracle.truth(name)
    whole, whole_gradient = forward_backward(device, name)
    alone, alone_gradient = forward_backward(
        device, name, x=want['x'][1:2], upstream=want['upstream'][1:2])
    assert torch.equal(whole[1:2], alone)
    assert torch.equal(whole_gradient[1:2], alone_gradient)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_three_dimensions_equal_two(device, name):
    want = oracle.truth(name)
    two, two_gradient = forward_backward(device, name)
    three, three_gradient = forward_backward(
        device, name, x=want['x'][:, None])
    assert three_gradient.shape == (oracle.BATCH, 1, want['x'].shape[1])
    assert torch.equal(two, three)
    assert torch.equal(two_gradient, three_gradient[:, 0])


@pytest.mark.gpu
def test_the_bands_are_views_of_the_transposed_magnitudes(device):
    want = oracle.truth('CMB')
    _, sizes, _ = oracle.CASES['CMB']
    x = want['x'].to(device)
    bands = discriminator.spectrogram_multiband(x)
    assert [b.shape[-1] for b in bands] == [51, 77, 128, 128, 129]
    base = bands[0]._base if bands[0]._base is not None else bands[0]
    start = base.data_ptr()
    for (low, _), band in zip(oracle.DEFAULT_EDGES, bands):
        assert band.shape[:3] == (oracle.BATCH, 1, oracle.FRAMES['CMB'])
        assert band.stride() == bands[0].stride()
        assert band.data_ptr() == start + 4 * low
    # the same magnitudes as the R-style output, transposed, to the bit
    plain = discriminator.spectrogram_resolution(x, sizes)
    assert torch.equal(torch.cat(bands, -1), plain.transpose(2, 3))
    # other bands, as fractions of the bins
    halves = discriminator.spectrogram_multiband(
        x, bands=((0., .5), (.5, 1.)))
    assert torch.equal(torch.cat(halves, -1), torch.cat(bands, -1))
    assert [b.shape[-1] for b in halves] == [256, 257]


###############################################################################
# DB
###############################################################################


@pytest.mark.gpu
@pytest.mark.parametrize('name', DECIBEL)
def test_swapped_rows_give_swapped_outputs(device, name):
    """One floor for the whole batch: a per-row maximum would floor nothing
    of the quiet row"""
    want = oracle.truth(name)
    out, gradient = forward_backward(device, name)
    swapped, swapped_gradient = forward_backward(
        device, name, x=want['x'].flip(0), upstream=want['upstream'].flip(0))
    assert torch.equal(swapped, out.flip(0))
    assert torch.equal(swapped_gradient, gradient.flip(0))
    assert (out[1] == out.min()).float().mean() > .2


@pytest.mark.gpu
@pytest.mark.parametrize('name', DECIBEL)
def test_zero_input_gives_a_zero_gradient(device, name):
    want = oracle.truth(name)
    out, gradient = forward_backward(
        device, name, x=torch.zeros_like(want['x']))
    # 20 log10(1e-5) everywhere: every element holds the maximum
    assert torch.equal(out, out.flatten()[0].expand_as(out))
    assert abs(out.flatten()[0].item() + 100.) < 1e-4
    assert torch.equal(gradient, torch.zeros_like(gradient))


###############################################################################
# All modes
###############################################################################


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_two_runs_are_bit_identical(device, name):
    first = forward_backward(device, name)
    second = forward_backward(device, name)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_forward_and_backward_capture_into_one_graph(device, name):
    want = oracle.truth(name)
    generator = torch.Generator().manual_seed(5)
    other = oracle.SIGMA * torch.randn(want['x'].shape, generator=generator)
    static = want['x'].to(device).requires_grad_(True)
    upstream = want['upstream'].to(device)

    def step():
        out = run(name, static)
        return out, torch.autograd.grad(
            out, static, upstream.reshape(out.shape))[0]

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, gradient = step()
    with torch.no_grad():
        static.copy_(other.to(device))
    graph.replay()
    torch.cuda.synchronize(device)
    replayed = out.clone(), gradient.clone()
    eager = step()
    assert torch.equal(replayed[0], eager[0])
    assert torch.equal(replayed[1], eager[1])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['R-512', 'CMB', 'DB-256'])
def test_bf16_input_returns_a_bf16_gradient(device, name):
    want = oracle.truth(name)
    leaf = want['x'].to(device, torch.bfloat16).requires_grad_(True)
    out = run(name, leaf)
    assert out.dtype == torch.float32
    upstream = want['upstream'].to(device).reshape(out.shape)
    out.backward(upstream)
    assert leaf.grad.dtype == torch.bfloat16
    # the same bits as the fp32 path on the rounded input, rounded once
    _, gradient = forward_backward(
        device, name, x=leaf.detach().float().cpu())
    assert torch.equal(leaf.grad, gradient.bfloat16())


@pytest.mark.gpu
def test_the_patched_methods_equal_the_functions(device):
    edges = [list(e) for e in oracle.DEFAULT_EDGES]

    def refuse(self, x):
        raise AssertionError('a device tensor went to the original method')

    module = types.SimpleNamespace(**{
        name: type(name, (), {'spectrogram': refuse})
        for name in ('DiscriminatorR', 'DiscriminatorCMB',
                     'SpecDiscriminatorBase')})
    discriminator.patch_module(module)
    cases = (
        ('R-1024', module.DiscriminatorR, {'resolution': (1024, 120, 600)}),
        ('CMB', module.DiscriminatorCMB,
         {'window_length': 1024, 'hop_size': 256, 'bands': edges}),
        ('DB-256', module.SpecDiscriminatorBase,
         {'resolution': [256, 64, 256]}))
    for name, cls, attributes in cases:
        instance = cls()
        vars(instance).update(attributes)
        x = oracle.truth(name)['x'].to(device)[:, None]
        got = instance.spectrogram(x)
        if name == 'CMB':
            assert isinstance(got, list) and len(got) == 5
            got = torch.cat(got, -1)
        assert torch.equal(got, run(name, x))
