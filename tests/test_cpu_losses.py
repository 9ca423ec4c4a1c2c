"""promonet_amd.loss without a GPU: the oracle (tests/losses_oracle.py) against
the golden from the reference and against autograd, the argument checks, the
ABI table, and the input conditions the GPU tests rely on."""
import re
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib

import losses_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = (
    'pm_sc_forward_workspace_bytes', 'pm_sc_adjoint_workspace_bytes',
    'pm_sc_stft', 'pm_sc_forward', 'pm_sc_adjoint',
    'pm_signal_loss_workspace_bytes', 'pm_signal_loss',
    'pm_signal_loss_backward')


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'losses.pt')


def relative(got, want):
    return ((got - want).abs().max() / want.abs().max()).item()


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('case', (0, 1))
def test_oracle_equals_the_reference_golden(golden, case):
    """fp64 against the reference run in fp64: 1e-9 relative; the gradients
    are stored as fp32, so they are held to fp32's rounding (2^-24) x 4."""
    key = f'case{case}/'
    batch, samples = golden[key + 'shape'].tolist()
    x, y = (t.double() for t in oracle.inputs(
        int(golden[key + 'seed']), batch, samples))
    assert relative(oracle.stft(x, 2560, 640, 2560),
                    golden[key + 'stft2560'].double()) < 4 * 2. ** -24
    for sizes, want in zip(oracle.DEFAULT_RESOLUTIONS,
                           golden[key + 'resolution_losses']):
        got = oracle.spectral_convergence(x, y, *sizes)
        assert relative(got, want) < 1e-9, sizes
    got = oracle.spectral_convergence(x, y, 1024, 120, 600)
    assert relative(got, golden[key + 'single_loss']) < 1e-9
    leaf = x.clone().requires_grad_(True)
    loss = oracle.multi_resolution(leaf, y)
    loss.backward()
    assert relative(loss.detach(), golden[key + 'loss']) < 1e-9
    assert relative(leaf.grad, golden[key + 'gradient'].double()) < 4 * 2. ** -24
    assert relative(oracle.signal(y, x), golden[key + 'signal']) < 1e-9
    assert relative(oracle.signal_gradient(y, x),
                    golden[key + 'signal_gradient'].double()) < 4 * 2. ** -24


@pytest.mark.parametrize('sizes,samples', (
    ((80, 20, 80), 203), ((80, 20, 80), 41), ((64, 16, 64), 130),
    ((1024, 120, 600), 1500), ((2560, 640, 2560), 1281)))
def test_hand_written_gradients_equal_autograd(sizes, samples):
    x, y = (t.double() for t in oracle.inputs(3, 2, samples))
    fft_size = sizes[0]
    # G against autograd of S1 by the spectrum
    X = oracle.transform(x, *sizes).detach().requires_grad_(True)
    s_y = oracle.stft(y, *sizes)
    (s_y - oracle.magnitude_root(X)).abs().sum().backward()
    G = oracle.bin_gradient(x, y, *sizes)
    assert relative(torch.view_as_real(G), torch.view_as_real(X.grad)) < 1e-12
    # the adjoint against autograd of <G, STFT(x)>, G with imaginary parts at
    # DC and Nyquist
    generator = torch.Generator().manual_seed(5)
    G = torch.randn(X.shape, dtype=torch.complex128, generator=generator)
    leaf = x.clone().requires_grad_(True)
    spectrum = oracle.transform(leaf, *sizes)
    (spectrum.real * G.real + spectrum.imag * G.imag).sum().backward()
    got = oracle.adjoint(G, samples, *sizes)
    assert relative(got, leaf.grad) < 1e-12
    # the two chained against autograd of the loss
    leaf = x.clone().requires_grad_(True)
    oracle.spectral_convergence(leaf, y, *sizes).backward()
    got = oracle.adjoint(
        oracle.bin_gradient(x, y, *sizes), samples, *sizes) / s_y.sum()
    assert relative(got, leaf.grad) < 1e-12
    assert fft_size // 2 + 1 == X.shape[1]
    assert 1 + samples // sizes[1] == X.shape[2]


def test_oracle_transform_is_torch_stft():
    x, _ = (t.double() for t in oracle.inputs(4, 2, 700))
    for fft_size, hop_size, win_length in ((1024, 120, 600), (80, 20, 80)):
        want = torch.stft(
            x, fft_size, hop_size, win_length,
            torch.hann_window(win_length, dtype=torch.float64),
            return_complex=True)
        got = oracle.transform(x, fft_size, hop_size, win_length)
        assert relative(torch.view_as_real(got), torch.view_as_real(want)) < 1e-13


def test_signal_gradient_equals_autograd_with_a_zero_row():
    x, y = (t.double() for t in oracle.inputs(2, 3, 500))
    x[1] = 0.
    leaf = x.clone().requires_grad_(True)
    loss = oracle.signal(y, leaf)
    loss.backward()
    assert torch.isfinite(leaf.grad).all()
    assert relative(oracle.signal_gradient(y, x), leaf.grad) < 1e-12
    # the zero row: p = 0, so its term of the mean is exactly 1
    assert oracle.signal(y[1:2], x[1:2]).item() == 1.


###############################################################################
# Argument checks (they answer before any device is touched)
###############################################################################


def test_value_errors_name_the_limit():
    loss = promonet_amd.loss
    for fft_size in (32, 96, 2048 + 1024, 5120, 63):
        with pytest.raises(ValueError, match='2\\^a or 5 \\* 2\\^a'):
            loss.SpectralConvergence('cpu', fft_size, 16, 32)
    for hop_size in (0, 1025):
        with pytest.raises(ValueError, match='hop_size'):
            loss.SpectralConvergence('cpu', 1024, hop_size, 600)
    with pytest.raises(ValueError, match='win_length'):
        loss.SpectralConvergence('cpu', 1024, 120, 1025)
    with pytest.raises(ValueError, match='window'):
        loss.SpectralConvergence('cpu', window='no_such_window')
    with pytest.raises(ValueError, match='2\\^a or 5 \\* 2\\^a'):
        loss.MultiResolutionSpectralConvergence(
            'cpu', [2560, 100], [640, 25], [2560, 100])
    module = loss.MultiResolutionSpectralConvergence('cpu')
    x = torch.zeros(2, 1, 1280)
    with pytest.raises(ValueError, match='reflect padding needs more than'):
        module(x, x)
    with pytest.raises(ValueError, match='differ in shape'):
        module(torch.zeros(2, 1, 4096), torch.zeros(2, 1, 4095))
    with pytest.raises(ValueError, match=r'\(B, 1, T\) or \(B, T\)'):
        module(torch.zeros(2, 2, 4096), torch.zeros(2, 2, 4096))
    window = torch.hann_window(80)
    with pytest.raises(ValueError, match='reflect padding needs more than'):
        loss.stft(torch.zeros(1, 40), 80, 20, 80, window)
    with pytest.raises(ValueError, match='win_length is 64'):
        loss.stft(torch.zeros(1, 400), 80, 20, 64, window)
    with pytest.raises(ValueError, match='same shape'):
        loss.signal(torch.zeros(2, 10), torch.zeros(2, 11))


def test_the_target_has_no_gradient():
    loss = promonet_amd.loss
    x = torch.zeros(1, 1, 4096)
    target = torch.zeros(1, 1, 4096, requires_grad=True)
    with pytest.raises(NotImplementedError, match='target is a constant'):
        loss.MultiResolutionSpectralConvergence('cpu')(x, target)
    with pytest.raises(NotImplementedError, match='target is a constant'):
        loss.SpectralConvergence('cpu')(x, target)
    with pytest.raises(NotImplementedError, match='y_true'):
        loss.signal(target, x)
    # ... and there is no CPU fallback behind the checks
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss.SpectralConvergence('cpu')(x, x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss.signal(x, x)


def test_abi_entries_and_their_argument_checks():
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    declared = set(re.findall(r'\b(pm_[a-z0-9_]+)\s*\(', header))
    library = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in declared, name
        assert hasattr(library, name), name
    # the workspace queries answer 0 outside the limits, the entries -1
    assert library.pm_sc_forward_workspace_bytes(2, 4096, 96, 24, 1) == 0
    assert library.pm_sc_forward_workspace_bytes(2, 1280, 2560, 640, 1) == 0
    assert library.pm_sc_adjoint_workspace_bytes(2, 4096, 80, 0) == 0
    def round256(size):
        return (size + 255) // 256 * 256
    # (frames of 80 floats; G as bins x frames complex fp32; both to 256 bytes)
    assert library.pm_sc_adjoint_workspace_bytes(2, 4096, 80, 20) == \
        round256(2 * 205 * 80 * 4)
    with_g = library.pm_sc_forward_workspace_bytes(3, 4096, 2560, 640, 1)
    without = library.pm_sc_forward_workspace_bytes(3, 4096, 2560, 640, 0)
    assert with_g - without == round256(3 * 1281 * 7 * 8)
    assert 0 < without <= 256
    assert library.pm_sc_stft(
        None, None, None, None, None, None, 1, 4096, 3072, 640, None) == -1
    assert b'fft_size' in library.pm_last_error()
    assert library.pm_sc_forward(
        None, None, None, None, None, 1, 1280, 2560, 640, 0, None, 0,
        None) == -1
    assert b'reflect' in library.pm_last_error()
    assert library.pm_sc_adjoint(
        None, None, None, None, None, 1, 4096, 80, 81, 0, None, 0,
        None) == -1
    assert b'hop_size' in library.pm_last_error()
    assert library.pm_signal_loss_workspace_bytes(0) == 0
    assert library.pm_signal_loss(None, None, None, 0, 5, None, 0, None) == -1


###############################################################################
# The input conditions of tests/test_gpu_losses.py
###############################################################################


def test_noise_inputs_leave_at_most_a_thousandth_of_the_bins_fragile():
    for sizes in oracle.CONFIGURATIONS:
        for batch, samples in oracle.shapes_of(sizes[0]):
            x, y = oracle.inputs(oracle.NOISE_SEED, batch, samples)
            share = oracle.fragile(x, y, *sizes).double().mean().item()
            assert share <= 1e-3, (sizes, batch, samples, share)


def test_end_to_end_inputs_have_no_fragile_bin_and_both_signs():
    for batch, samples in oracle.SHAPES:
        x, y = oracle.scaled_inputs(oracle.END_TO_END_SEED, batch, samples)
        for sizes in oracle.DEFAULT_RESOLUTIONS:
            assert not oracle.fragile(x, y, *sizes).any(), (samples, sizes)
        if batch > 1:
            difference = oracle.stft(y.double(), 80, 20, 80) - \
                oracle.stft(x.double(), 80, 20, 80)
            assert (difference[0] > 0).all() and (difference[1] < 0).all()


def test_every_configuration_runs_its_shapes():
    # the shortest row N = 2560 admits is among the shapes, with three frames
    assert (2, 1281) in oracle.shapes_of(2560)
    assert 1 + 1281 // 640 == 3
    for sizes in oracle.CONFIGURATIONS:
        assert len(oracle.shapes_of(sizes[0])) >= 3
    for fft_size in (64, 80, 160):
        assert (2, fft_size // 2 + 1) in oracle.shapes_of(fft_size)


def test_gates_stay_within_four_times_the_fp32_restatement():
    """No capped gate of test_gpu_losses.py exceeds 4x the figure the float32
    CPU restatement reaches on the same inputs (the largest over the cases),
    and every gate lies between its measurement and 3x that."""
    import test_gpu_losses as gpu
    worst = {}
    for sizes, shape in gpu.CASES:
        for kind, figure in gpu.fp32_figures(sizes, shape).items():
            worst[kind] = max(worst.get(kind, 0.), figure)
    worst['end_to_end'] = max(
        gpu.end_to_end_truth(shape, True)['fp32'] for shape in oracle.SHAPES)
    worst['end_to_end_noise'] = max(
        gpu.end_to_end_truth(shape, False)['fp32'] for shape in oracle.SHAPES)
    worst['signal'] = max(
        gpu.signal_fp32_figure(shape) for shape in gpu.SIGNAL_SHAPES)
    assert set(worst) == set(gpu.GATES)
    for kind, (gate, measured) in gpu.GATES.items():
        print(f'{kind}: gate {gate}, measured {measured}, '
              f'fp32 CPU {worst[kind]:.4g}')
        if kind in gpu.CAPPED:
            assert gate <= 4 * worst[kind], (kind, gate, worst[kind])
        # 3x the measurement, or less where the cap binds; never under it
        assert measured < gate <= 3.001 * measured, kind
