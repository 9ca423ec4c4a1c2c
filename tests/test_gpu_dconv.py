"""The conv stacks of the complex multi-band and the multi-resolution
discriminators on the device (promonet_amd.model.discriminator: band_conv,
weight_norm, DiscriminatorCMB, DiscriminatorR) against the float64 oracle
(tests/dconv_oracle.py) and the reference's own run (tests/golden/dconv.pt).

Gates: per quantity (forward, gx, gW, gb) 4 x the largest error that the
reference's own arithmetic in fp32 (conv2d + leaky_relu with autograd on the
build host's CPU) shows against the same oracle over the case table, relative
to each case's RMS (oracle.FP32_RECORDED). The gates stand on the recorded CPU
figures, never on the device's.
"""
import types
from pathlib import Path

import pytest
import torch

from promonet_amd import loss
from promonet_amd.model import discriminator

import conv_checks
import dconv_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
ALL_NAMES = list(oracle.ALL_CASES)
STACKS = ('cmb', 'r')
pytestmark = pytest.mark.gpu


def layer(name, x, weight, bias):
    _, _, _, stride, _, _, slope = oracle.ALL_CASES[name]
    return discriminator.band_conv(x, weight, bias, stride, slope)


FAMILY = conv_checks.Family(
    oracle, lambda name, x, weight, bias, rows: layer(name, x, weight, bias))


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'dconv.pt')


###############################################################################
# Within the gate
###############################################################################


@pytest.mark.parametrize('name', ALL_NAMES)
def test_a_layer_is_within_the_gate(device, name):
    channels, out_channels, _, stride, height, width, _ = \
        oracle.ALL_CASES[name]
    got = FAMILY.result(device, name)
    assert got[0].shape == (
        oracle.BATCH, out_channels, height, (width - 1) // stride + 1)
    assert got[1].shape == (oracle.BATCH, channels, height, width)
    conv_checks.a_layer_is_within_the_gate(FAMILY, device, name)


@pytest.mark.parametrize('shape', oracle.WEIGHT_NORM_SHAPES)
def test_weight_norm_is_within_the_gate(device, shape):
    """The existing weight norm at fan 27, 288 and 864"""
    conv_checks.weight_norm_is_within_the_gate(oracle, device, shape)


###############################################################################
# The modules
###############################################################################


def golden_module(golden, device, name):
    module = discriminator.DiscriminatorCMB() if name == 'cmb' \
        else discriminator.DiscriminatorR(golden['resolution'])
    assert list(module.state_dict()) == golden['keys'][name]
    module.load_state_dict(oracle.parameters(name))
    return module.to(device)


def stack_inputs(name, x):
    if name == 'cmb':
        return [x[..., low:high] for low, high in oracle.CMB_EDGES]
    return x


@pytest.mark.parametrize('name', STACKS)
def test_the_module_gives_the_golden_within_the_gate(device, golden, name):
    module = golden_module(golden, device, name)
    x = golden['stacks'][name]['x'].to(device).requires_grad_(True)
    logits, maps = module.stack(stack_inputs(name, x))
    assert len(maps) == (26 if name == 'cmb' else 6) and maps[-1] is logits
    total = sum((c.to(device) * o).sum() for c, o in zip(
        oracle.golden_coefficients(golden, name), maps))
    total.backward()
    gradients = {key: value.grad.cpu()
                 for key, value in module.named_parameters()}
    figures = oracle.stack_figures(
        golden, name, logits.detach().cpu(),
        [m.detach().cpu() for m in maps[:-1]], x.grad.cpu(), gradients)
    print(' '.join(f'{label} {value:.3e}' for label, _, value in figures))
    for label, quantity, value in figures:
        assert value < oracle.gate(quantity), (label, value)


def test_forward_from_audio_equals_the_stack_on_the_spectrogram(device):
    audio = .1 * torch.randn(
        2, 1, 4096, generator=torch.Generator().manual_seed(3)).to(device)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        cmb = discriminator.DiscriminatorCMB().to(device)
        res = discriminator.DiscriminatorR((512, 50, 240)).to(device)
    leaf = audio.clone().requires_grad_(True)
    logits, maps = cmb(leaf)
    want, want_maps = cmb.stack(discriminator.spectrogram_multiband(audio))
    assert len(maps) == 26 and logits.ndim == 2
    assert torch.equal(logits, torch.flatten(want, 1, -1))
    for got, expected in zip(maps, want_maps):
        assert torch.equal(got, expected)
    logits.sum().backward()
    assert leaf.grad.shape == audio.shape and leaf.grad.abs().sum() > 0.
    logits, maps = res(audio)
    want, want_maps = res.stack(
        discriminator.spectrogram_resolution(audio, (512, 50, 240)))
    assert len(maps) == 6
    assert torch.equal(logits, torch.flatten(want, 1, -1))
    for got, expected in zip(maps, want_maps):
        assert torch.equal(got, expected)


@pytest.mark.parametrize('name', STACKS)
def test_the_maps_reach_feature_matching_without_a_copy(device, golden, name):
    module = golden_module(golden, device, name)
    x = golden['stacks'][name]['x']
    with torch.no_grad():
        real = module.stack(stack_inputs(name, x.to(device)))[1]
        fake = module.stack(stack_inputs(name, (x + 1.).to(device)))[1]
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
    # n < 2^18 terms a map moves by far less than n 2^-24 of itself)
    assert torch.allclose(direct, copied, rtol=1e-4, atol=0.)


###############################################################################
# Also
###############################################################################


@pytest.mark.parametrize('name', ALL_NAMES)
def test_two_runs_are_bit_identical(device, name):
    conv_checks.two_runs_are_bit_identical(FAMILY, device, name)


@pytest.mark.parametrize('name', ['first', 'large', 'layer5', 'post'])
def test_forward_and_backward_capture_into_one_graph(device, name):
    conv_checks.forward_and_backward_capture_into_one_graph(
        FAMILY, device, name)


@pytest.mark.parametrize('name', ['first', 'odd-width', 'post'])
def test_zero_input_gives_the_bias(device, name):
    conv_checks.zero_input_gives_the_bias(
        FAMILY, device, name, oracle.CASES[name][6])


@pytest.mark.parametrize(
    'name', ['first', 'even-width', 'large', 'post', 'walked'])
def test_a_row_alone_equals_the_row_in_its_batch(device, name):
    conv_checks.a_row_alone_equals_the_row_in_its_batch(FAMILY, device, name)


@pytest.mark.parametrize('name', ['first', 'odd-width', 'post'])
def test_bf16_input_returns_a_bf16_gradient(device, name):
    conv_checks.bf16_input_returns_a_bf16_gradient(FAMILY, device, name)


def test_autocast_computes_in_fp32(device):
    conv_checks.autocast_computes_in_fp32(FAMILY, device, 'odd-width')


def test_a_band_slice_and_its_copy_give_the_same(device):
    want = oracle.truth('first')
    wide = torch.randn(2, 1, 5, 80, generator=torch.Generator().manual_seed(2))
    wide[..., 10:61] = want['x']
    view = wide.to(device)[..., 10:61]
    assert not view.is_contiguous()
    arguments = [want[k].to(device) for k in ('weight', 'bias')]
    assert torch.equal(layer('first', view, *arguments),
                       layer('first', want['x'].to(device), *arguments))


###############################################################################
# patch(): stand-ins with the reference's layer layout
###############################################################################


def conv(*args, **kwargs):
    return torch.nn.utils.weight_norm(torch.nn.Conv2d(*args, **kwargs))


def stand_in(stride=(1, 2)):
    """DiscriminatorCMB (two bands) and DiscriminatorR with the reference's
    layer layout; stride (2, 1) is a form the kernels do not compute"""
    calls = []

    def convs():
        return [conv(1, 32, (3, 9), (1, 1), padding=(1, 4)),
                conv(32, 32, (3, 9), stride, padding=(1, 4)),
                conv(32, 32, (3, 9), (1, 2), padding=(1, 4)),
                conv(32, 32, (3, 9), (1, 2), padding=(1, 4)),
                conv(32, 32, (3, 3), (1, 1), padding=(1, 1))]

    class DiscriminatorCMB(torch.nn.Module):

        def __init__(self):
            super().__init__()
            self.window_length, self.hop_size = 256, 64
            self.bands = [(0, 40), (40, 129)]
            self.band_convs = torch.nn.ModuleList([
                torch.nn.ModuleList([
                    torch.nn.Sequential(c, torch.nn.LeakyReLU(0.1))
                    for c in convs()]) for _ in self.bands])
            self.conv_post = conv(32, 1, (3, 3), (1, 1), padding=(1, 1))

        def spectrogram(self, x):
            return discriminator._multiband(
                x, self.window_length, self.hop_size, self.bands)

        def forward(self, x):
            calls.append('cmb')
            x_bands = self.spectrogram(x)
            x, fmap = [], []
            for band, stack in zip(x_bands, self.band_convs):
                for entry in stack:
                    band = entry(band)
                    fmap.append(band)
                x.append(band)
            x = self.conv_post(torch.cat(x, dim=-1))
            fmap.append(x)
            return torch.flatten(x, 1, -1), fmap

    class DiscriminatorR(torch.nn.Module):

        def __init__(self, resolution):
            super().__init__()
            self.resolution = resolution
            self.convs = torch.nn.ModuleList(convs())
            self.conv_post = conv(32, 1, (3, 3), padding=(1, 1))

        def spectrogram(self, x):
            return discriminator.spectrogram_resolution(x, self.resolution)

        def forward(self, audio):
            calls.append('r')
            x, fmap = self.spectrogram(audio), []
            for entry in self.convs:
                x = torch.nn.functional.leaky_relu(entry(x), 0.2)
                fmap.append(x)
            x = self.conv_post(x)
            fmap.append(x)
            return torch.flatten(x, 1, -1), fmap

    return types.SimpleNamespace(
        DiscriminatorCMB=DiscriminatorCMB, DiscriminatorR=DiscriminatorR), calls


def test_the_patched_modules_equal_the_functions(device):
    module, calls = stand_in()
    originals = (module.DiscriminatorCMB.forward, module.DiscriminatorR.forward)
    discriminator.patch_module(module)
    discriminator.patch_module(module)
    assert module.DiscriminatorCMB.forward.original is originals[0]
    assert module.DiscriminatorR.forward.original is originals[1]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        cmb = module.DiscriminatorCMB().to(device)
        res = module.DiscriminatorR((256, 64, 256)).to(device)
    audio = .1 * torch.randn(
        2, 1, 2048, generator=torch.Generator().manual_seed(4)).to(device)

    logits, maps = cmb(audio)
    assert not calls and len(maps) == 11
    expected, last = [], []
    for band, stack in zip(cmb.spectrogram(audio), cmb.band_convs):
        for entry in stack:
            band = discriminator.band_conv(
                band, discriminator.weight_norm(
                    entry[0].weight_g, entry[0].weight_v), entry[0].bias,
                entry[0].stride, 0.1)
            expected.append(band)
        last.append(band)
    expected.append(discriminator.band_conv(
        torch.cat(last, dim=-1), discriminator.weight_norm(
            cmb.conv_post.weight_g, cmb.conv_post.weight_v),
        cmb.conv_post.bias))
    assert torch.equal(logits, torch.flatten(expected[-1], 1, -1))
    for got, want in zip(maps, expected):
        assert torch.equal(got, want)
    theirs, their_maps = originals[0](cmb, audio)
    assert calls == ['cmb']
    assert torch.allclose(logits, theirs, rtol=1e-3, atol=1e-4)
    assert [m.shape for m in maps] == [m.shape for m in their_maps]

    logits, maps = res(audio)
    assert calls == ['cmb'] and len(maps) == 6
    x, expected = res.spectrogram(audio), []
    for entry in list(res.convs) + [res.conv_post]:
        x = discriminator.band_conv(
            x, discriminator.weight_norm(entry.weight_g, entry.weight_v),
            entry.bias, entry.stride, 1. if entry is res.conv_post else 0.2)
        expected.append(x)
    assert torch.equal(logits, torch.flatten(expected[-1], 1, -1))
    for got, want in zip(maps, expected):
        assert torch.equal(got, want)
    theirs, _ = originals[1](res, audio)
    assert calls == ['cmb', 'r']
    assert torch.allclose(logits, theirs, rtol=1e-3, atol=1e-4)


def test_a_stack_of_another_form_goes_to_the_original(device):
    module, calls = stand_in(stride=(2, 1))
    discriminator.patch_module(module)
    audio = .1 * torch.randn(
        2, 1, 2048, generator=torch.Generator().manual_seed(4)).to(device)
    module.DiscriminatorCMB().to(device)(audio)
    module.DiscriminatorR((256, 64, 256)).to(device)(audio)
    assert calls == ['cmb', 'r']
