"""The strided, wider layers of the FARGAN discriminator's conv stacks on the
device (promonet_amd.model.discriminator: frequency_conv(stride=),
DiscriminatorMagFree(strided=True)) against the float64 oracle
(tests/fdisc_strided_oracle.py) and the reference's own run
(tests/golden/fdisc_strided.pt).

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
import fdisc_strided_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
SIZES = (128, 256, 512, 1024, 2048)
pytestmark = pytest.mark.gpu


def layer(name, x, weight, bias, **kwargs):
    _, _, _, _, stride, activation = oracle.CASES[name]
    return discriminator.frequency_conv(
        x, weight, bias, 1, activation, stride=stride, **kwargs)


FAMILY = conv_checks.Family(
    oracle, lambda name, x, weight, bias, rows: layer(name, x, weight, bias))


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'fdisc_strided.pt')


###############################################################################
# Within the gate
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_a_layer_is_within_the_gate(device, name):
    channels, out_channels, bins, frames, stride, _ = oracle.CASES[name]
    got = FAMILY.result(device, name)
    assert got[0].shape == (
        oracle.BATCH, out_channels, (bins - 1) // stride + 1, frames)
    assert got[1].shape == (oracle.BATCH, channels, bins, frames)
    conv_checks.a_layer_is_within_the_gate(FAMILY, device, name)


###############################################################################
# The module
###############################################################################


def hashed_module(n_fft, device):
    module = discriminator.DiscriminatorMagFree(
        [n_fft, n_fft // 4, n_fft], strided=True)
    module.load_state_dict(dict(
        oracle.parameters(n_fft),
        filterbank=torch.zeros_like(module.state_dict()['filterbank'])))
    return module.to(device)


@pytest.mark.parametrize('n_fft', SIZES)
def test_the_module_gives_the_golden_within_the_gate(device, golden, n_fft):
    kept = golden['stacks'][n_fft]
    module = hashed_module(n_fft, device)
    x = kept['x'].to(device).requires_grad_(True)
    logits, maps = module.stack(x)
    assert [list(m.shape) for m in maps + [logits]] == kept['shapes']
    total = sum((c.to(device) * o).sum() for c, o in zip(
        oracle.coefficients(kept['shapes']), maps + [logits]))
    total.backward()
    report = []

    def within(label, got, want, quantity):
        value = oracle.figure(got.detach().cpu(), want)
        report.append(f'{label} {value:.3e}')
        assert value < oracle.gate(quantity), (label, value)

    try:
        within('logits', logits, kept['logits'], 'forward')
        for index, (got, want) in enumerate(zip(maps, kept['maps'])):
            # (flattened in the logical order, whatever the memory order)
            within(f'map{index}',
                   got.contiguous().flatten()[::golden['map_stride']], want,
                   'forward')
        within('gx', x.grad.flatten()[::golden['input_stride']],
               kept['gradient_x'], 'gx')
        named = dict(module.named_parameters())
        for key, want in kept['gradients'].items():
            step = golden['gradient_stride'] if key.endswith('weight_v') else 1
            within(key, named[key].grad.flatten()[::step], want,
                   'gb' if key.endswith('bias') else 'gW')
    finally:
        print(f'{n_fft}: ' + ' '.join(report))


def test_the_maps_reach_feature_matching_without_a_copy(device, golden):
    module = hashed_module(256, device)
    x = golden['stacks'][256]['x']
    real = module.stack(x.to(device))[1]
    fake = module.stack((x + 1.).to(device))[1]
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
    # at most 16 896 terms a map moves by far less than n 2^-24 = 1e-3 of
    # itself)
    assert torch.allclose(direct, copied, rtol=1e-5, atol=0.)


def test_forward_from_audio_has_the_reference_s_shapes(device):
    module = discriminator.DiscriminatorMagFree(
        [512, 128, 512], strided=True).to(device)
    audio = .1 * torch.randn(
        2, 1, 2048, generator=torch.Generator().manual_seed(3)).to(device)
    audio.requires_grad_(True)
    logits, maps = module(audio)
    frames = 1 + 2048 // 128
    assert logits.shape == (2, 33 * frames)
    assert [tuple(m.shape) for m in maps] == [
        (2, 16, 129, frames), (2, 32, 65, frames), (2, 64, 33, frames),
        (2, 128, 33, frames), (2, 128, 33, frames)]
    logits.sum().backward()
    assert audio.grad.shape == audio.shape and audio.grad.abs().sum() > 0.


###############################################################################
# Also
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_two_runs_are_bit_identical(device, name):
    conv_checks.two_runs_are_bit_identical(FAMILY, device, name)


@pytest.mark.parametrize('name', ['first-even', 'large', 'square', 'last'])
def test_forward_and_backward_capture_into_one_graph(device, name):
    conv_checks.forward_and_backward_capture_into_one_graph(
        FAMILY, device, name)


@pytest.mark.parametrize('name', ['first-odd', 'two-bins', 'widest', 'last'])
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


@pytest.mark.parametrize('name', ['first-even', 'square', 'large', 'last'])
def test_a_row_alone_equals_the_row_in_its_batch(device, name):
    conv_checks.a_row_alone_equals_the_row_in_its_batch(FAMILY, device, name)


@pytest.mark.parametrize('name', ['first-odd', 'one-frame', 'last'])
def test_bf16_input_returns_a_bf16_gradient(device, name):
    conv_checks.bf16_input_returns_a_bf16_gradient(FAMILY, device, name)


def test_the_new_entries_serve_the_narrow_forms(device):
    """(16, 16, 1) through pm_fdisc_layer_* is pm_fdisc_conv_*'s result"""
    generator = torch.Generator().manual_seed(9)
    x = torch.randn(2, 16, 9, 5, generator=generator).to(device)
    weight = torch.randn(16, 18, 3, 3, generator=generator).to(device)
    bias = torch.randn(16, generator=generator).to(device)
    table = discriminator._embedding_table(x.device, 9)
    want = discriminator.frequency_conv(x, weight, bias)
    got = discriminator._ConvLayer.apply(
        x, weight, bias, discriminator._STRIDED_ENTRIES, (2, 16, 16, 9, 5, 1),
        (1,), table)
    assert torch.equal(got, want)


###############################################################################
# patch(): a stand-in with the reference's layer layout at n_fft 256
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


def stand_in():
    calls = []

    class SpecDiscriminatorBase(torch.nn.Module):

        def __init__(self, resolution):
            super().__init__()
            self.resolution = resolution
            layers = []
            for index, (stride, _, channels, out) in enumerate(
                    discriminator.magfree_plan(resolution[0])):
                layers.append(torch.nn.Sequential(
                    FrequencyPositionalEmbedding(),
                    torch.nn.utils.weight_norm(torch.nn.Conv2d(
                        channels + 2, out, (3, 3), stride=(stride, 1),
                        dilation=(1, 1), padding=(1, 1))),
                    torch.nn.Sigmoid() if index == 5
                    else torch.nn.ReLU(inplace=True)))
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
            conv.bias, 1, 'sigmoid' if index == 5 else 'relu',
            stride=conv.stride[0])
        expected.append(x)
    assert [m.shape[2] for m in expected] == [65, 33, 33, 33, 33, 33]
    assert torch.equal(logits, torch.flatten(expected[-1], 1, -1))
    assert len(maps) == 5
    for got, want in zip(maps, expected):
        assert torch.equal(got, want)
    # ... and is close to the original method on torch's own ops
    theirs, _ = original(model, audio)
    assert calls == ['original']
    assert torch.allclose(logits, theirs, rtol=1e-3, atol=1e-4)
