"""The convs of the generator's MRF Blocks on the device, both ways
(promonet_amd.model.hifigan_train: block_conv, Block, ResidualBlock,
HiFiGANTrainable, patch_module) against the float64 oracle
(tests/gconv_oracle.py).

Gates: per quantity (forward, gx, gW, gb) 4 x the largest error that the
reference's own arithmetic in fp32 (leaky_relu and conv1d with autograd on the
build host's CPU) shows against the same oracle over the case table, relative
to each case's RMS (oracle.FP32_RECORDED); the modules and the whole vocoder
likewise on the fp32 CPU run of their compositions (oracle.MODULE_RECORDED,
oracle.TRAINABLE_RECORDED). The gates stand on the recorded CPU figures, never
on the device's.
"""
import types

import pytest
import torch

import promonet_amd
from promonet_amd.model import discriminator, hifigan_train

import conv_checks
import gconv_oracle as oracle

NAMES = list(oracle.CASES)
LARGE = ['form-32-11-5', 'form-256-11-5', 'short-64-26', 'large-32',
         'large-128']
pytestmark = pytest.mark.gpu


def layer(name, x, weight, bias, slope, residual=None):
    return hifigan_train.block_conv(
        x, weight, bias, oracle.CASES[name][2], slope, residual)


def case_layer(case, x, weight, bias, rows):
    name, slope, residual = case
    return layer(name, x, weight, bias, slope, oracle.truth(name, slope)[
        'residual'][rows].to(x.device) if residual else None)


# a case of the shared bodies: (name, slope, with the residual)
FAMILY = conv_checks.Family(
    oracle, case_layer, truth=lambda case: oracle.truth(*case[:2]),
    figures=lambda case, *got: oracle.figures(
        *case[:2], *got, residual=case[2]),
    recorded=lambda case: oracle.FP32_RECORDED[case[0]],
    label=lambda case: f'{case[0]} slope {case[1]} residual {case[2]}')


###############################################################################
# Within the gate
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_a_layer_is_within_the_gate(device, name):
    for slope in oracle.SLOPES:
        for residual in (False, True):
            conv_checks.a_layer_is_within_the_gate(
                FAMILY, device, (name, slope, residual))


def test_the_output_is_a_view_of_channels_last_memory(device):
    want = oracle.truth('form-32-3-1', oracle.SLOPE)
    x = want['x'].to(device).requires_grad_(True)
    y = layer('form-32-3-1', x, want['weight'].to(device),
              want['bias'].to(device), oracle.SLOPE)
    assert y.shape == x.shape and y.transpose(1, 2).is_contiguous()
    # such a view is taken without a copy, and any strides give the same bits
    again = layer('form-32-3-1', hifigan_train.channels_last(x.detach()),
                  want['weight'].to(device), want['bias'].to(device),
                  oracle.SLOPE)
    assert torch.equal(y, again)
    y.backward(want['upstream'].to(device))
    assert x.grad.shape == x.shape


###############################################################################
# The modules
###############################################################################


def module_of(name, device):
    if name == 'residual':
        module = hifigan_train.ResidualBlock(oracle.MODULE_CHANNELS)
    else:
        kernel = int(name.split('-')[1])
        module = hifigan_train.Block(
            oracle.MODULE_CHANNELS, kernel, dict(oracle.BLOCKS)[kernel])
    want = oracle.module_truth(name)
    assert list(module.state_dict()) == list(want['parameters'])
    module.load_state_dict(want['parameters'])
    return module.to(device)


@pytest.mark.parametrize('name', list(oracle.MODULE_SEEDS))
def test_a_module_is_within_the_gate(device, name):
    want = oracle.module_truth(name)
    module = module_of(name, device)
    x = want['x'].to(device).requires_grad_(True)
    y = module(x)
    y.backward(want['upstream'].to(device))
    figures = oracle.module_figures(
        name, y.detach().cpu(), x.grad.cpu(),
        {key: value.grad.cpu() for key, value in module.named_parameters()})
    print(f'{name}: device ' + ' '.join(f'{v:.3e}' for v in figures) +
          ' fp32 CPU recorded ' +
          ' '.join(f'{v:.3e}' for v in oracle.MODULE_RECORDED[name]))
    for value, limit in zip(figures, oracle.module_gates()):
        assert value < limit, (value, limit)


def test_a_block_equals_the_hand_composition(device):
    want = oracle.module_truth('block-7')
    module = module_of('block-7', device)
    x = want['x'].to(device)
    expected = x
    for c1, c2, d in zip(module.convs1, module.convs2, (1, 3, 5)):
        xt = hifigan_train.block_conv(
            expected, discriminator.weight_norm(c1.weight_g, c1.weight_v),
            c1.bias, d, oracle.SLOPE)
        expected = hifigan_train.block_conv(
            xt, discriminator.weight_norm(c2.weight_g, c2.weight_v), c2.bias,
            1, oracle.SLOPE, residual=expected)
    assert torch.equal(module(x), expected)


@pytest.fixture(scope='module')
def trainable(device):
    state = oracle.trainable_state()
    module = hifigan_train.HiFiGANTrainable(113, 258)
    module.load_state_dict(state, strict=True)
    return module.to(device)


def test_the_vocoder_is_within_the_gate(device, trainable):
    features, global_features, upstream = oracle.trainable_inputs()
    x = features.to(device).requires_grad_(True)
    g = global_features.to(device).requires_grad_(True)
    trainable.zero_grad()
    y = trainable(x, g)
    assert y.shape == upstream.shape
    y.backward(upstream.to(device))
    figures = oracle.trainable_figures(
        y.detach().cpu(), x.grad.cpu(), g.grad.cpu(),
        {key: value.grad.cpu() for key, value in trainable.named_parameters()})
    print('vocoder: device ' + ' '.join(f'{v:.3e}' for v in figures) +
          ' fp32 CPU recorded ' +
          ' '.join(f'{v:.3e}' for v in oracle.TRAINABLE_RECORDED))
    for value, limit in zip(figures, oracle.trainable_gates()):
        assert value < limit, (value, limit)


def test_the_state_dict_round_trips_with_hifigan(device, trainable):
    promonet_amd.configure(COMPUTE_DTYPE='fp32')
    try:
        engine = promonet_amd.model.HiFiGAN(113, 258)
    finally:
        promonet_amd.configure(
            COMPUTE_DTYPE=promonet_amd.config.DEFAULT_COMPUTE_DTYPE)
    state = trainable.state_dict()
    assert list(state) == list(engine.state_dict())
    assert all(p.requires_grad for p in trainable.parameters())
    engine.load_state_dict(state, strict=True)
    other = hifigan_train.HiFiGANTrainable(113, 258)
    other.load_state_dict(engine.state_dict(), strict=True)
    for key, value in other.state_dict().items():
        assert torch.equal(value.cpu(), state[key].cpu()), key
    # the same state, the inference engine with exact fp32 operands
    engine = engine.to(device).eval()
    features, global_features, _ = oracle.trainable_inputs()
    with torch.no_grad():
        want = engine(features.to(device), global_features.to(device))
        got = trainable(features.to(device), global_features.to(device))
    value = oracle.figure(got.cpu(), want.cpu())
    print(f'trainable against the engine in fp32: {value:.3e}')
    assert value < oracle.trainable_gates()[0]


###############################################################################
# Also
###############################################################################


@pytest.mark.parametrize('name', LARGE)
def test_two_runs_are_bit_identical(device, name):
    conv_checks.two_runs_are_bit_identical(
        FAMILY, device, (name, oracle.SLOPE, True))


@pytest.mark.parametrize('name', LARGE)
def test_a_row_alone_equals_the_row_in_its_batch(device, name):
    conv_checks.a_row_alone_equals_the_row_in_its_batch(
        FAMILY, device, (name, oracle.SLOPE, True))


@pytest.mark.parametrize('name', LARGE)
def test_zero_input_gives_the_bias_and_the_residual(device, name):
    want = oracle.truth(name, oracle.SLOPE)
    bias, residual = want['bias'].to(device), want['residual'].to(device)
    zeros = torch.zeros_like(want['x']).to(device)
    y = layer(name, zeros, want['weight'].to(device), bias, oracle.SLOPE)
    assert torch.equal(y, bias[None, :, None].expand_as(y))
    y = layer(name, zeros, want['weight'].to(device), bias, oracle.SLOPE,
              residual)
    assert torch.equal(y, bias[None, :, None] + residual)


@pytest.mark.parametrize('name', ['form-256-11-5', 'large-32', 'large-128'])
def test_forward_and_backward_capture_into_one_graph(device, name):
    want = oracle.truth(name, oracle.SLOPE)
    generator = torch.Generator().manual_seed(5)
    other = torch.randn(want['x'].shape, generator=generator)
    static = want['x'].to(device).requires_grad_(True)
    weight = want['weight'].to(device).requires_grad_(True)
    bias = want['bias'].to(device).requires_grad_(True)
    residual = want['residual'].to(device)
    upstream = want['upstream'].to(device)

    def step():
        out = layer(name, static, weight, bias, oracle.SLOPE, residual)
        return (out,) + torch.autograd.grad(
            out, (static, weight, bias), upstream)

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outputs = step()
    with torch.no_grad():
        static.copy_(other.to(device))
    graph.replay()
    torch.cuda.synchronize(device)
    replayed = [t.clone() for t in outputs]
    for a, b in zip(replayed, step()):
        assert torch.equal(a, b)


@pytest.mark.parametrize('needs', [
    (True, False, False, False), (False, True, False, False),
    (False, False, True, False), (False, False, False, True),
    (True, False, False, True), (False, True, True, False)])
def test_the_subsets_of_the_gradients(device, needs):
    name = 'form-64-7-3'
    want = oracle.truth(name, oracle.SLOPE)
    whole = FAMILY.result(device, (name, oracle.SLOPE, True))
    leaves = [want[key].to(device).requires_grad_(need) for key, need in zip(
        ('x', 'weight', 'bias', 'residual'), needs)]
    y = layer(name, *leaves[:3], oracle.SLOPE, leaves[3])
    y.backward(want['upstream'].to(device))
    expected = list(whole[1:]) + [want['upstream']]
    for leaf, need, value in zip(leaves, needs, expected):
        if need:
            assert torch.equal(leaf.grad.cpu(), value)
        else:
            assert leaf.grad is None


def test_bf16_input_returns_a_bf16_gradient(device):
    name = 'form-32-7-1'
    want = oracle.truth(name, oracle.SLOPE)
    leaf = want['x'].to(device, torch.bfloat16).requires_grad_(True)
    residual = want['residual'].to(device, torch.bfloat16).requires_grad_(True)
    arguments = [want[key].to(device) for key in ('weight', 'bias')]
    y = layer(name, leaf, *arguments, oracle.SLOPE, residual)
    assert y.dtype == torch.float32
    y.backward(want['upstream'].to(device))
    assert leaf.grad.dtype == torch.bfloat16 and leaf.grad.shape == leaf.shape
    assert residual.grad.dtype == torch.bfloat16
    exact = layer(name, leaf.detach().float(), *arguments, oracle.SLOPE,
                  residual.detach().float())
    assert torch.equal(y, exact)


def test_autocast_computes_in_fp32(device):
    conv_checks.autocast_computes_in_fp32(
        FAMILY, device, ('form-128-3-1', oracle.SLOPE, False))


###############################################################################
# patch(): a stand-in with the reference's layer layout
###############################################################################


def conv(channels, kernel, dilation, padding=None):
    return torch.nn.utils.weight_norm(torch.nn.Conv1d(
        channels, channels, kernel, 1, dilation=dilation,
        padding=(kernel - 1) // 2 * dilation if padding is None else padding))


def stand_in():
    """Block with the reference's layer layout (:157-210)"""
    calls = []

    class Block(torch.nn.Module):

        def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
            super().__init__()
            self.convs1 = torch.nn.ModuleList(
                [conv(channels, kernel_size, d) for d in dilation])
            self.convs2 = torch.nn.ModuleList(
                [conv(channels, kernel_size, 1) for _ in dilation])
            self.activations1, self.activations2 = (
                torch.nn.ModuleList(
                    [torch.nn.LeakyReLU(negative_slope=.1) for _ in dilation])
                for _ in range(2))

        def forward(self, x):
            calls.append('block')
            for c1, c2, a1, a2 in zip(self.convs1, self.convs2,
                                      self.activations1, self.activations2):
                x = c2(a2(c1(a1(x)))) + x
            return x

    return types.SimpleNamespace(Block=Block), calls


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_the_patched_block_equals_the_functions(device):
    module, calls = stand_in()
    original = module.Block.forward
    hifigan_train.patch_module(module)
    hifigan_train.patch_module(module)
    assert module.Block.forward.original is original
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        member = module.Block(64, 7).to(device)
    x = torch.randn(
        2, 64, 50, generator=torch.Generator().manual_seed(4)).to(device)
    leaf = x.clone().requires_grad_(True)
    y = member(leaf)
    assert not calls
    expected = x
    for c1, c2 in zip(member.convs1, member.convs2):
        xt = hifigan_train.block_conv(
            expected, discriminator.weight_norm(c1.weight_g, c1.weight_v),
            c1.bias, c1.dilation[0], .1)
        expected = hifigan_train.block_conv(
            xt, discriminator.weight_norm(c2.weight_g, c2.weight_v), c2.bias,
            1, .1, residual=expected)
    assert torch.equal(y, expected)
    y.sum().backward()
    assert leaf.grad.shape == x.shape
    assert all(p.grad is not None for p in member.parameters())
    theirs = original(member, x)
    assert calls == ['block']
    assert torch.allclose(y, theirs, rtol=1e-3, atol=1e-4)
    # autograd off: the original
    with torch.no_grad():
        member(x)
    assert calls == ['block'] * 2


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_a_block_of_another_form_goes_to_the_original(device):
    module, calls = stand_in()
    hifigan_train.patch_module(module)
    x = torch.randn(
        2, 48, 50, generator=torch.Generator().manual_seed(4)).to(device)
    module.Block(48, 3).to(device)(x)
    assert calls == ['block']
    module.Block(32, 5).to(device)(x[:, :32])
    assert calls == ['block'] * 2
    module.Block(32, 3, (1, 2, 4)).to(device)(x[:, :32])
    assert calls == ['block'] * 3
