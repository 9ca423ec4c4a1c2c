"""promonet_amd.loss on the GPU against the float64 oracle
(tests/losses_oracle.py), stage by stage through the C ABI and end to end
through autograd.

Every gate is K x an error model of an fp32 transform (delta = 2^-24 log2(N)
|windowed frame|_2 per frame). Each K is 3x the largest figure measured on an
MI355X (GATES below lists the measurements), and may not exceed 4x the figure
the float32 CPU restatement reaches on the same inputs: each test prints that
figure beside its own, and test_cpu_losses.py asserts the bound over all cases.

Two gates are not plain 3x figures:
  end_to_end (y = c_b x, no fragile bin): measured 1.616e-5 relative L2, the
    float32 CPU restatement reaches 9.21e-6, so 3x measured (4.85e-5) would
    pass the cap of 4 x 9.21e-6 = 3.68e-5: the cap binds and the gate is 3.4e-5,
    2.1x the measurement. The figure is carried by the few bins of smallest
    |X| (G grows as |X|^-1.5), where the error of X is what two fp32
    transforms differ in; the rows of the restatement itself range from 2.2e-6
    to 9.2e-6.
  end_to_end_noise (independent x and y): the gate as measured, 3 x 2.081e-4,
    with the fragile bins counted (14, 3 and 2 per shape). One flipped sign
    moves the L2 error by about 1 / sqrt(bins), so the float32 restatement's
    own figure (6.7e-5) is no bound for it and the cap is not applied.
"""
import ctypes
import functools
import math
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib

import losses_oracle as oracle
from util import check

ROOT = Path(__file__).resolve().parent.parent
EPS = 2. ** -24

# gate: (K, largest figure measured on the MI355X); K = 3 x measured
GATES = {
    'transform': (4.9, 1.633),
    'loss': (7.05, 2.351),
    'bin_gradient': (3.07, 1.025),
    'adjoint': (1.24, 0.4137),
    'end_to_end': (3.4e-5, 1.616e-5),
    'end_to_end_noise': (6.24e-4, 2.081e-4),
    'signal': (0.805, 0.2684),
}
# the gates held to 4x the float32 CPU restatement (see the docstring)
CAPPED = tuple(kind for kind in GATES if kind != 'end_to_end_noise')

CASES = [(sizes, shape) for sizes in oracle.CONFIGURATIONS
         for shape in oracle.shapes_of(sizes[0])]
CASE_IDS = [f'{s[0]}-{s[1]}-{s[2]}-B{b}-T{t}' for s, (b, t) in CASES]


def gate(kind):
    return GATES[kind][0]


###############################################################################
# The figures: an error in units of its model (shared with the fp32 CPU
# restatement, so that the two are compared like for like)
###############################################################################


@functools.lru_cache(maxsize=None)
def truth(sizes, shape, seed=oracle.NOISE_SEED):
    """Everything the fp64 oracle says about a case, computed once"""
    x, y = oracle.inputs(seed, *shape)
    xd, yd = x.double(), y.double()
    X = oracle.transform(xd, *sizes)
    out = {'x': x, 'y': y, 'X': X, 's': oracle.magnitude_root(X),
           'delta': oracle.delta(x, *sizes),
           'loss': oracle.spectral_convergence(xd, yd, *sizes),
           'G': oracle.bin_gradient(xd, yd, *sizes),
           'fragile': oracle.fragile(x, y, *sizes)}
    generator = torch.Generator().manual_seed(11)
    out['random_G'] = torch.randn(
        X.shape, dtype=torch.complex64, generator=generator)
    out['adjoint'] = oracle.adjoint(
        out['random_G'].to(torch.complex128), shape[1], *sizes)
    return out


def figure_transform(s, want):
    return ((s.double() - want['s']).abs() * 2 * want['s']
            / want['delta']).max().item()


def figure_loss(loss, want):
    return abs(float(loss) - float(want)) / float(want) / EPS


def figure_bin_gradient(G, want):
    keep = ~want['fragile']
    error = (G.to(torch.complex128) - want['G']).abs()
    unit = 1.5 * want['delta'] / want['X'].abs() * want['G'].abs()
    return (error[keep] / unit[keep]).max().item()


def figure_l2(got, want, unit=1.):
    """largest relative L2 error of a row, over `unit`"""
    got, want = got.double(), want.double()
    return ((got - want).norm(dim=-1) / want.norm(dim=-1)).max().item() / unit


@functools.lru_cache(maxsize=None)
def fp32_figures(sizes, shape):
    """The figures of the float32 CPU restatement on a case's inputs"""
    want = truth(sizes, shape)
    x, y = want['x'], want['y']
    return {
        'transform': figure_transform(oracle.stft(x, *sizes), want),
        'loss': figure_loss(
            oracle.spectral_convergence(x, y, *sizes), want['loss']),
        'bin_gradient': figure_bin_gradient(
            oracle.bin_gradient(x, y, *sizes), want),
        'adjoint': figure_l2(
            oracle.adjoint(want['random_G'], shape[1], *sizes),
            want['adjoint'], EPS * math.log2(sizes[0]))}


def oracle_gradient(x, y, dtype):
    leaf = x.to(dtype).clone().requires_grad_(True)
    loss = oracle.multi_resolution(leaf, y.to(dtype))
    loss.backward()
    return loss.detach(), leaf.grad


@functools.lru_cache(maxsize=None)
def end_to_end_truth(shape, scaled):
    if scaled:
        x, y = oracle.scaled_inputs(oracle.END_TO_END_SEED, *shape)
    else:
        x, y = oracle.inputs(oracle.NOISE_SEED, *shape)
    loss, gradient = oracle_gradient(x, y, torch.float64)
    loss32, gradient32 = oracle_gradient(x, y, torch.float32)
    fragile = sum(int(oracle.fragile(x, y, *sizes).sum())
                  for sizes in oracle.DEFAULT_RESOLUTIONS)
    return {'x': x, 'y': y, 'loss': loss, 'gradient': gradient,
            'fp32': figure_l2(gradient32, gradient), 'fragile': fragile}


def signal_figures(value, gradient, y_true, y_pred):
    want = oracle.signal(y_true.double(), y_pred.double())
    want_gradient = oracle.signal_gradient(y_true.double(), y_pred.double())
    unit = EPS * math.sqrt(y_pred.shape[-1])
    return max(abs(float(value) - float(want)) / abs(float(want)) / unit,
               figure_l2(gradient, want_gradient, unit))


###############################################################################
# Helpers around the ABI
###############################################################################


def tables(device, sizes):
    fft_size, _, win_length = sizes
    return (promonet_amd.loss._named_window(
                device, 'hann_window', win_length, fft_size),
            promonet_amd.loss._twiddle(device, fft_size))


def forward_with_gradient(device, x, y, sizes):
    """pm_sc_forward through the ABI: sums (3) and G read from the workspace"""
    library = _lib.lib()
    window, twiddle = tables(device, sizes)
    x, y = x.to(device), y.to(device)
    batch, samples = x.shape
    fft_size, hop_size, _ = sizes
    size = library.pm_sc_forward_workspace_bytes(
        batch, samples, fft_size, hop_size, 1)
    workspace = torch.zeros(size, dtype=torch.uint8, device=device)
    sums = torch.empty(3, device=device)
    _lib.check(library.pm_sc_forward(
        _lib.ptr(x), _lib.ptr(y), _lib.ptr(window), _lib.ptr(twiddle),
        _lib.ptr(sums), batch, samples, fft_size, hop_size, 1,
        workspace.data_ptr(), size, _lib.stream()))
    bins, frames = fft_size // 2 + 1, 1 + samples // hop_size
    G = workspace[:batch * bins * frames * 8].view(torch.float32).view(
        batch, bins, frames, 2)
    return sums.cpu(), torch.view_as_complex(G.cpu().contiguous())


def adjoint_through_abi(device, G, samples, sizes, into=None):
    library = _lib.lib()
    window, twiddle = tables(device, sizes)
    fft_size, hop_size, _ = sizes
    batch = G.shape[0]
    flat = torch.view_as_real(G).contiguous().to(device)
    out = torch.empty(batch, samples, device=device) if into is None \
        else into.to(device).clone()
    scale = torch.ones(1, device=device)
    size = library.pm_sc_adjoint_workspace_bytes(
        batch, samples, fft_size, hop_size)
    workspace = torch.empty(size, dtype=torch.uint8, device=device)
    _lib.check(library.pm_sc_adjoint(
        _lib.ptr(flat), _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(scale),
        _lib.ptr(out), batch, samples, fft_size, hop_size,
        int(into is not None), workspace.data_ptr(), size, _lib.stream()))
    return out.cpu()


###############################################################################
# 1-4: the stages
###############################################################################


@pytest.mark.gpu
@pytest.mark.parametrize('sizes,shape', CASES, ids=CASE_IDS)
def test_transform(device, sizes, shape):
    want = truth(sizes, shape)
    window = torch.hann_window(sizes[2], dtype=torch.float64).float()
    s = promonet_amd.loss.stft(
        want['x'].to(device), *sizes, window.to(device)).cpu()
    assert s.shape == want['s'].shape and s.dtype == torch.float32
    figure = figure_transform(s, want)
    print(f'transform {sizes} {shape}: {figure:.3f} delta/2s '
          f'(fp32 CPU {fp32_figures(sizes, shape)["transform"]:.3f})')
    check(figure, gate('transform'), 'loss/transform', (sizes, shape))


@pytest.mark.gpu
@pytest.mark.parametrize('sizes,shape', CASES, ids=CASE_IDS)
def test_loss_and_bin_gradient(device, sizes, shape):
    want = truth(sizes, shape)
    sums, G = forward_with_gradient(device, want['x'], want['y'], sizes)
    fp32 = fp32_figures(sizes, shape)
    figure = figure_loss(sums[2], want['loss'])
    print(f'loss {sizes} {shape}: {figure:.3f} x 2^-24 '
          f'(fp32 CPU {fp32["loss"]:.3f})')
    check(figure, gate('loss'), 'loss/loss', (sizes, shape))
    # (the quotient is taken in double on the device, before one rounding)
    assert abs(float(sums[2]) - float(sums[0]) / float(sums[1])) \
        <= 4 * EPS * float(sums[2])
    # the module agrees with the ABI to the bit, with and without a gradient
    module = promonet_amd.loss.SpectralConvergence(device, *sizes)
    x, y = want['x'].to(device), want['y'].to(device)
    assert module(x, y).item() == float(sums[2])
    assert module(x.clone().requires_grad_(True), y).item() == float(sums[2])
    share = want['fragile'].double().mean().item()
    assert share <= 1e-3, share
    figure = figure_bin_gradient(G, want)
    print(f'bin gradient {sizes} {shape}: {figure:.3f} x 1.5 delta/|X| |G| '
          f'(fp32 CPU {fp32["bin_gradient"]:.3f}), fragile share {share:.2e}')
    check(figure, gate('bin_gradient'), 'loss/bin_gradient', (sizes, shape))


@pytest.mark.gpu
@pytest.mark.parametrize('case', (0, 1))
def test_losses_equal_the_golden(device, case):
    golden = torch.load(ROOT / 'tests' / 'golden' / 'losses.pt')
    key = f'case{case}/'
    batch, samples = golden[key + 'shape'].tolist()
    x, y = (t.to(device) for t in oracle.inputs(
        int(golden[key + 'seed']), batch, samples))
    loss = promonet_amd.loss
    figures = [figure_loss(loss.SpectralConvergence(device, *sizes)(x, y), want)
               for sizes, want in zip(oracle.DEFAULT_RESOLUTIONS,
                                      golden[key + 'resolution_losses'])]
    figures.append(figure_loss(
        loss.SpectralConvergence(device)(x[:, None], y[:, None]),
        golden[key + 'single_loss']))
    figures.append(figure_loss(
        loss.MultiResolutionSpectralConvergence(device)(x, y),
        golden[key + 'loss']))
    print(f'golden case {case}: {figures} x 2^-24')
    check(max(figures), gate('loss'), 'loss/loss', ('golden', case))


@pytest.mark.gpu
@pytest.mark.parametrize('sizes,shape', CASES, ids=CASE_IDS)
def test_adjoint(device, sizes, shape):
    want = truth(sizes, shape)
    G = want['random_G']
    assert G[:, 0].imag.abs().min() > 0 and G[:, -1].imag.abs().min() > 0
    unit = EPS * math.log2(sizes[0])
    got = adjoint_through_abi(device, G, shape[1], sizes)
    figure = figure_l2(got, want['adjoint'], unit)
    start = torch.randn(shape, generator=torch.Generator().manual_seed(13))
    summed = adjoint_through_abi(device, G, shape[1], sizes, into=start)
    # accumulate adds the same bits to what was there, in one fp32 add
    assert torch.equal(summed, start + got)
    print(f'adjoint {sizes} {shape}: {figure:.3f} x 2^-24 log2 N '
          f'(fp32 CPU {fp32_figures(sizes, shape)["adjoint"]:.3f})')
    check(figure, gate('adjoint'), 'loss/adjoint', (sizes, shape))


###############################################################################
# 5: end to end
###############################################################################


def gradient_on_device(device, x, y, module=None):
    module = module or promonet_amd.loss.MultiResolutionSpectralConvergence(
        device)
    leaf = x.to(device).requires_grad_(True)
    loss = module(leaf, y.to(device))
    loss.backward()
    return loss.detach().cpu(), leaf.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', oracle.SHAPES)
def test_end_to_end(device, shape):
    want = end_to_end_truth(shape, True)
    assert want['fragile'] == 0
    loss, gradient = gradient_on_device(device, want['x'], want['y'])
    figure = figure_l2(gradient, want['gradient'])
    print(f'end to end {shape}: {figure:.3e} relative L2 '
          f'(fp32 CPU {want["fp32"]:.3e})')
    check(figure, gate('end_to_end'), 'loss/end_to_end', shape)
    check(figure_loss(loss, want['loss']), gate('loss'), 'loss/loss', shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', oracle.SHAPES)
def test_end_to_end_independent_noise(device, shape):
    want = end_to_end_truth(shape, False)
    loss, gradient = gradient_on_device(device, want['x'], want['y'])
    figure = figure_l2(gradient, want['gradient'])
    print(f'end to end, noise {shape}: {figure:.3e} relative L2 with '
          f'{want["fragile"]} fragile bins (fp32 CPU {want["fp32"]:.3e})')
    check(figure, gate('end_to_end_noise'), 'loss/end_to_end_noise', shape)
    check(figure_loss(loss, want['loss']), gate('loss'), 'loss/loss', shape)


@pytest.mark.gpu
def test_zero_input_has_a_zero_gradient(device):
    _, y = oracle.inputs(oracle.NOISE_SEED, 2, 4096)
    x = torch.zeros_like(y)
    loss, gradient = gradient_on_device(device, x, y)
    assert torch.equal(gradient, torch.zeros_like(gradient))
    want = oracle.multi_resolution(x.double(), y.double())
    check(figure_loss(loss, want), gate('loss'), 'loss/loss', 'zero input')


###############################################################################
# 6: determinism and plumbing
###############################################################################


@pytest.mark.gpu
def test_runs_are_bit_identical_and_shapes_agree(device):
    x, y = oracle.inputs(oracle.NOISE_SEED, 3, 4099)
    module = promonet_amd.loss.MultiResolutionSpectralConvergence(device)
    first = gradient_on_device(device, x, y, module)
    second = gradient_on_device(device, x, y, module)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])
    third = gradient_on_device(device, x[:, None], y[:, None], module)
    assert third[1].shape == (3, 1, 4099)
    assert torch.equal(first[0], third[0])
    assert torch.equal(first[1], third[1][:, 0])


@pytest.mark.gpu
def test_a_row_does_not_depend_on_its_batch(device):
    x, _ = oracle.inputs(oracle.NOISE_SEED, 3, 4099)
    x = x.to(device)
    for sizes in ((80, 20, 80), (1024, 120, 600), (2560, 640, 2560)):
        window = torch.hann_window(sizes[2], device=device)
        whole = promonet_amd.loss.stft(x, *sizes, window)
        alone = promonet_amd.loss.stft(x[1:2], *sizes, window)
        assert torch.equal(whole[1:2], alone), sizes


@pytest.mark.gpu
def test_bf16_input_returns_a_bf16_gradient(device):
    x, y = oracle.inputs(oracle.NOISE_SEED, 2, 4096)
    leaf = x.to(device, torch.bfloat16).requires_grad_(True)
    module = promonet_amd.loss.MultiResolutionSpectralConvergence(device)
    loss = module(leaf, y.to(device, torch.bfloat16))
    loss.backward()
    assert loss.dtype == torch.float32 and loss.ndim == 0
    assert leaf.grad.dtype == torch.bfloat16
    # the same bits as the fp32 path on the rounded input, rounded once
    _, want = gradient_on_device(
        device, leaf.detach().float().cpu(), y.bfloat16().float(), module)
    assert torch.equal(leaf.grad.cpu(), want.bfloat16())


@pytest.mark.gpu
def test_stft_is_differentiable(device):
    sizes = (320, 80, 320)
    x, _ = oracle.inputs(oracle.NOISE_SEED, 2, 1281)
    leaf = x.to(device).requires_grad_(True)
    window = torch.hann_window(320, device=device)
    weights = torch.randn(
        2, 161, 17, generator=torch.Generator().manual_seed(3))
    (promonet_amd.loss.stft(leaf, *sizes, window)
     * weights.to(device)).sum().backward()
    reference = x.double().requires_grad_(True)
    (oracle.stft(reference, *sizes) * weights.double()).sum().backward()
    # the chain G -> adjoint, under the end-to-end gate of the noise inputs
    # (the weights put no bin's sign at stake, its phase only)
    check(figure_l2(leaf.grad.cpu(), reference.grad),
          gate('end_to_end_noise'), 'loss/stft_backward', sizes)


@pytest.mark.gpu
def test_forward_and_backward_capture_into_one_graph(device):
    x, y = oracle.inputs(oracle.NOISE_SEED, 2, 4096)
    other, _ = oracle.inputs(oracle.NOISE_SEED + 1, 2, 4096)
    module = promonet_amd.loss.MultiResolutionSpectralConvergence(device)
    static = x.to(device).requires_grad_(True)
    target = y.to(device)

    def step():
        loss = module(static, target) + promonet_amd.loss.signal(
            target, static)
        return loss, torch.autograd.grad(loss, static)[0]

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, gradient = step()
    with torch.no_grad():
        static.copy_(other.to(device))
    graph.replay()
    torch.cuda.synchronize(device)
    replayed = loss.clone(), gradient.clone()
    eager = step()
    assert torch.equal(replayed[0], eager[0])
    assert torch.equal(replayed[1], eager[1])


###############################################################################
# 7: signal
###############################################################################


SIGNAL_SHAPES = ((3, 4096), (1, 4099), (5, 1, 257))


def signal_inputs(shape):
    """y_true, y_pred; row 1 of y_pred is zeros where there is one"""
    generator = torch.Generator().manual_seed(17)
    y_true = .1 * torch.randn(shape, generator=generator)
    y_pred = y_true + .05 * torch.randn(shape, generator=generator)
    if shape[0] > 1:
        y_pred[1] = 0.
    return y_true, y_pred


def signal_fp32_figure(shape):
    y_true, y_pred = signal_inputs(shape)
    return signal_figures(
        oracle.signal(y_true, y_pred), oracle.signal_gradient(y_true, y_pred),
        y_true, y_pred)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SIGNAL_SHAPES)
def test_signal(device, shape):
    y_true, y_pred = signal_inputs(shape)
    leaf = y_pred.to(device).requires_grad_(True)
    value = promonet_amd.loss.signal(y_true.to(device), leaf)
    value.backward()
    assert value.ndim == 0 and torch.isfinite(leaf.grad).all()
    figure = signal_figures(
        value.detach().cpu(), leaf.grad.cpu(), y_true, y_pred)
    print(f'signal {shape}: {figure:.3f} x 2^-24 sqrt T '
          f'(fp32 CPU {signal_fp32_figure(shape):.3f})')
    check(figure, gate('signal'), 'loss/signal', shape)
    if shape[0] > 1:
        # the zero row's loss is exactly 1, its gradient the oracle's
        alone = promonet_amd.loss.signal(
            y_true[1:2].to(device), y_pred[1:2].to(device))
        assert alone.item() == 1.
    again = y_pred.to(device).requires_grad_(True)
    promonet_amd.loss.signal(y_true.to(device), again).backward()
    assert torch.equal(again.grad, leaf.grad)
