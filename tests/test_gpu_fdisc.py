"""The conv stacks of the FARGAN discriminator on the device
(promonet_amd.model.discriminator: frequency_conv, weight_norm,
DiscriminatorMagFree) against the float64 oracle (tests/fdisc_oracle.py).

Gates: per quantity (forward, gx, gW, gb) 4 x the largest error that the
reference's own arithmetic in fp32 (torch.cat + conv2d + the activation, with
autograd, on the build host's CPU) shows against the same oracle over the case
table, relative to each case's RMS (oracle.FP32_RECORDED). The gates stand on
the recorded CPU figures, never on the device's.
"""
import types
from pathlib import Path

import pytest
import torch

from promonet_amd import loss
from promonet_amd.model import discriminator

import conv_checks
import fdisc_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
pytestmark = pytest.mark.gpu


def layer(name, x, weight, bias, **kwargs):
    _, _, _, _, dilation, activation = oracle.CASES[name]
    return discriminator.frequency_conv(
        x, weight, bias, dilation, activation, **kwargs)


FAMILY = conv_checks.Family(
    oracle, lambda name, x, weight, bias, rows: layer(name, x, weight, bias))


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'fdisc.pt')


###############################################################################
# Within the gate
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_a_layer_is_within_the_gate(device, name):
    channels, out_channels, bins, frames, _, _ = oracle.CASES[name]
    got = FAMILY.result(device, name)
    assert got[0].shape == (oracle.BATCH, out_channels, bins, frames)
    assert got[1].shape == (oracle.BATCH, channels, bins, frames)
    conv_checks.a_layer_is_within_the_gate(FAMILY, device, name)


@pytest.mark.parametrize('shape', [(16, 18, 3, 3), (16, 3, 3, 3),
                                   (1, 18, 3, 3)])
def test_weight_norm_is_within_the_gate(device, shape):
    conv_checks.weight_norm_is_within_the_gate(oracle, device, shape)


###############################################################################
# The module
###############################################################################


def golden_module(golden, device):
    """The reference's stack at n_fft = 64, the one resolution whose layers
    the kernels compute, with the golden's parameters"""
    kept = golden['stacks'][0]
    module = discriminator.DiscriminatorMagFree(kept['resolution'])
    state = module.state_dict()
    assert list(state) == golden['keys'][kept['resolution'][0]]
    module.load_state_dict(dict(kept['parameters'], filterbank=torch.zeros_like(
        state['filterbank'])))
    return module.to(device), kept


def test_the_module_gives_the_golden_within_the_gate(device, golden):
    module, kept = golden_module(golden, device)
    x = kept['x'].to(device).requires_grad_(True)
    logits, maps = module.stack(x)
    total = sum((c.to(device) * o).sum() for c, o in zip(
        oracle.coefficients(*logits.shape[::2], logits.shape[3]),
        maps + [logits]))
    total.backward()
    stride = golden['map_stride']
    report = []

    def within(label, got, want, quantity):
        value = oracle.figure(got.detach().cpu(), want)
        report.append(f'{label} {value:.3e}')
        assert value < oracle.gate(quantity), (label, value)

    try:
        within('logits', logits, kept['logits'], 'forward')
        for index, (got, want) in enumerate(zip(maps, kept['maps'])):
            # (flattened in the logical order, whatever the memory order)
            within(f'map{index}', got.contiguous().flatten()[::stride], want,
                   'forward')
        within('gx', x.grad, kept['gradient_x'], 'gx')
        named = dict(module.named_parameters())
        for key, want in kept['gradients'].items():
            step = golden['gradient_stride'] if key.endswith('weight_v') else 1
            within(key, named[key].grad.flatten()[::step], want,
                   'gb' if key.endswith('bias') else 'gW')
    finally:
        print(' '.join(report))


def test_the_maps_reach_feature_matching_without_a_copy(device, golden):
    module, kept = golden_module(golden, device)
    real = module.stack(kept['x'].to(device))[1]
    fake = module.stack((kept['x'] + 1.).to(device))[1]
    for r, f in zip(real, fake):
        assert r.stride() == f.stride() and r.shape == f.shape
        assert loss._dense(r) and loss._dense(f)
        pair = loss._adv_pair(r, f)
        assert pair[0].data_ptr() == r.data_ptr()
        assert pair[1].data_ptr() == f.data_ptr()
    direct = loss.feature_matching([real], [fake])
    copied = loss.feature_matching(
        [[r.contiguous() for r in real]], [[f.contiguous() for f in fake]])
    # (the two orders in memory add the same terms in another order: a sum of
    # n = 5 280 terms a map moves by far less than n 2^-24 = 3e-4 of itself)
    assert torch.allclose(direct, copied, rtol=1e-5, atol=0.)


def test_forward_from_audio_has_the_reference_s_shapes(device):
    module = discriminator.DiscriminatorMagFree([64, 16, 64]).to(device)
    audio = .1 * torch.randn(
        2, 1, 1024, generator=torch.Generator().manual_seed(3)).to(device)
    audio.requires_grad_(True)
    logits, maps = module(audio)
    frames = 1 + 1024 // 16
    assert logits.shape == (2, 33 * frames)
    assert [tuple(m.shape) for m in maps] == [(2, 16, 33, frames)] * 5
    logits.sum().backward()
    assert audio.grad.shape == audio.shape and audio.grad.abs().sum() > 0.


###############################################################################
# Also
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_two_runs_are_bit_identical(device, name):
    conv_checks.two_runs_are_bit_identical(FAMILY, device, name)


@pytest.mark.parametrize('name', ['first', 'large', 'last'])
def test_forward_and_backward_capture_into_one_graph(device, name):
    conv_checks.forward_and_backward_capture_into_one_graph(
        FAMILY, device, name)


@pytest.mark.parametrize('name', ['first', 'd2', 'last'])
def test_zero_input_and_zero_embedding_weights_give_the_bias(device, name):
    want = oracle.truth(name)
    channels = oracle.CASES[name][0]
    weight = want['weight'].clone()
    weight[:, channels:] = 0.
    bias = want['bias'].to(device)
    y = layer(name, torch.zeros_like(want['x']).to(device), weight.to(device),
              bias)
    if oracle.CASES[name][5] == 'relu':
        expected = bias.clamp(min=0.)[None, :, None, None].expand_as(y)
        assert torch.equal(y, expected)
    else:
        # one value at every pixel, the sigmoid of the bias to an ulp
        assert torch.equal(y, y[:1, :, :1, :1].expand_as(y))
        assert torch.allclose(
            y[0, :, 0, 0].double().cpu(),
            torch.sigmoid(want['bias'].double()), rtol=2. ** -22, atol=0.)


@pytest.mark.parametrize('name', ['first', 'd16', 'last'])
def test_a_row_alone_equals_the_row_in_its_batch(device, name):
    conv_checks.a_row_alone_equals_the_row_in_its_batch(FAMILY, device, name)


@pytest.mark.parametrize('name', ['first', 'd2', 'last'])
def test_bf16_input_returns_a_bf16_gradient(device, name):
    conv_checks.bf16_input_returns_a_bf16_gradient(FAMILY, device, name)


def test_autocast_computes_in_fp32(device):
    conv_checks.autocast_computes_in_fp32(FAMILY, device, 'd2')


###############################################################################
# patch(): a stand-in with the reference's layer layout
###############################################################################


class FrequencyPositionalEmbedding(torch.nn.Module):

    def forward(self, x):
        bins = x.size(2)
        args = torch.arange(
            0, bins, dtype=x.dtype, device=x.device) * torch.pi * 2 / bins
        cos = torch.cos(args).reshape(1, 1, -1, 1)
        sin = torch.sin(args).reshape(1, 1, -1, 1)
        zeros = torch.zeros_like(x[:, 0:1, :, :])
        return torch.cat((x, zeros + sin, zeros + cos), dim=1)


def stand_in(stride=1, dilations=(1, 2, 4, 4, 4, 4)):
    """SpecDiscriminatorBase with the reference's layer layout; the default
    dilations are a form the kernels compute that the reference does not
    build, stride 2 one they do not compute"""
    calls = []

    class SpecDiscriminatorBase(torch.nn.Module):

        def __init__(self, resolution):
            super().__init__()
            self.resolution = resolution
            layers, channels = [], 1
            for index, dilation in enumerate(dilations):
                out = 1 if index == 5 else 16
                layers.append(torch.nn.Sequential(
                    FrequencyPositionalEmbedding(),
                    torch.nn.utils.weight_norm(torch.nn.Conv2d(
                        channels + 2, out, (3, 3),
                        stride=(stride if index == 2 else 1, 1),
                        dilation=(dilation, 1), padding=(dilation, 1))),
                    torch.nn.Sigmoid() if index == 5
                    else torch.nn.ReLU(inplace=True)))
                channels = out
            self.layers = torch.nn.ModuleList(layers)

        def forward(self, x):
            calls.append('original')
            x = self.spectrogram(x).unsqueeze(1)
            output = []
            for entry in self.layers:
                x = entry(x)
                output.append(x)
            return torch.flatten(output[-1], 1, -1), output[:-1]

        def spectrogram(self, x):
            return discriminator.spectrogram_decibel(x, self.resolution)

    return types.SimpleNamespace(
        SpecDiscriminatorBase=SpecDiscriminatorBase), calls


def test_the_patched_module_equals_the_functions(device):
    module, calls = stand_in()
    original = module.SpecDiscriminatorBase.forward
    discriminator.patch_module(module)
    discriminator.patch_module(module)
    assert module.SpecDiscriminatorBase.forward.original is original
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        model = module.SpecDiscriminatorBase([256, 64, 256]).to(device)
    audio = .1 * torch.randn(
        2, 1, 1024, generator=torch.Generator().manual_seed(4)).to(device)
    logits, maps = model(audio)
    assert not calls
    x = discriminator.spectrogram_decibel(audio, [256, 64, 256]).unsqueeze(1)
    expected = []
    for index, entry in enumerate(model.layers):
        conv = entry[1]
        x = discriminator.frequency_conv(
            x, discriminator.weight_norm(conv.weight_g, conv.weight_v),
            conv.bias, conv.dilation[0], 'sigmoid' if index == 5 else 'relu')
        expected.append(x)
    assert torch.equal(logits, torch.flatten(expected[-1], 1, -1))
    assert len(maps) == 5
    for got, want in zip(maps, expected):
        assert torch.equal(got, want)
    # ... and is close to the original method on torch's own ops
    theirs, their_maps = original(model, audio)
    assert calls == ['original']
    assert torch.allclose(logits, theirs, rtol=1e-3, atol=1e-4)
    # a CPU tensor goes to the original method
    with pytest.raises(RuntimeError):
        model.cpu()(audio.cpu())
    assert calls == ['original', 'original']


def test_a_stack_of_another_form_goes_to_the_original(device):
    module, calls = stand_in(stride=2)
    discriminator.patch_module(module)
    model = module.SpecDiscriminatorBase([128, 32, 128]).to(device)
    audio = .1 * torch.randn(
        2, 1, 1024, generator=torch.Generator().manual_seed(4)).to(device)
    model(audio)
    assert calls == ['original']
