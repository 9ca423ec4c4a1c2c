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

import dconv_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
ALL_NAMES = list(oracle.ALL_CASES)
STACKS = ('cmb', 'r')
pytestmark = pytest.mark.gpu

_RESULTS = {}


def layer(name, x, weight, bias):
    _, _, _, stride, _, _, slope = oracle.ALL_CASES[name]
    return discriminator.band_conv(x, weight, bias, stride, slope)


def forward_backward(device, name, rows=slice(None)):
    """(y, gx, gW, gb) of the case on the device, on the CPU"""
    want = oracle.truth(name)
    x = want['x'][rows].to(device).requires_grad_(True)
    weight = want['weight'].to(device).requires_grad_(True)
    bias = want['bias'].to(device).requires_grad_(True)
    y = layer(name, x, weight, bias)
    y.backward(want['upstream'][rows].to(device))
    return tuple(t.detach().cpu() for t in (y, x.grad, weight.grad, bias.grad))


def result(device, name):
    if name not in _RESULTS:
        _RESULTS[name] = forward_backward(device, name)
    return _RESULTS[name]


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
    got = result(device, name)
    assert got[0].shape == (
        oracle.BATCH, out_channels, height, (width - 1) // stride + 1)
    assert got[1].shape == (oracle.BATCH, channels, height, width)
    figures = oracle.figures(name, *got)
    print(f'{name}: device ' + ' '.join(f'{v:.3e}' for v in figures) +
          ' fp32 CPU recorded ' +
          ' '.join(f'{v:.3e}' for v in oracle.FP32_RECORDED.get(name, ())))
    for quantity, value in zip(oracle.QUANTITIES, figures):
        assert value < oracle.gate(quantity), (quantity, value)


@pytest.mark.parametrize('shape', oracle.WEIGHT_NORM_SHAPES)
def test_weight_norm_is_within_the_gate(device, shape):
    """The existing weight norm at fan 27, 288 and 864"""
    g, v, upstream = oracle.weight_norm_inputs(shape)
    want = oracle.weight_norm(g, v)
    want_g, want_v = oracle.weight_norm_backward(upstream, g, v)
    leaf_g = g.to(device).requires_grad_(True)
    leaf_v = v.to(device).requires_grad_(True)
    w = discriminator.weight_norm(leaf_g, leaf_v)
    w.backward(upstream.to(device))
    figures = (oracle.figure(w.detach().cpu(), want),
               oracle.figure(leaf_g.grad.cpu(), want_g),
               oracle.figure(leaf_v.grad.cpu(), want_v))
    print(f'{shape}: device ' + ' '.join(f'{v:.3e}' for v in figures))
    for value, limit in zip(figures, oracle.WEIGHT_NORM_GATES):
        assert value < limit, (value, limit)


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
    first = result(device, name)
    second = forward_backward(device, name)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', ['first', 'large', 'layer5', 'post'])
def test_forward_and_backward_capture_into_one_graph(device, name):
    want = oracle.truth(name)
    generator = torch.Generator().manual_seed(5)
    other = torch.randn(want['x'].shape, generator=generator)
    static = want['x'].to(device).requires_grad_(True)
    weight = want['weight'].to(device).requires_grad_(True)
    bias = want['bias'].to(device).requires_grad_(True)
    upstream = want['upstream'].to(device)

    def step():
        out = layer(name, static, weight, bias)
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


@pytest.mark.parametrize('name', ['first', 'odd-width', 'post'])
def test_zero_input_gives_the_bias(device, name):
    want = oracle.truth(name)
    slope = oracle.CASES[name][6]
    bias = want['bias'].to(device)
    y = layer(name, torch.zeros_like(want['x']).to(device),
              want['weight'].to(device), bias)
    expected = torch.where(bias > 0., bias, bias * slope)
    assert torch.equal(y, expected[None, :, None, None].expand_as(y))


@pytest.mark.parametrize(
    'name', ['first', 'even-width', 'large', 'post', 'walked'])
def test_a_row_alone_equals_the_row_in_its_batch(device, name):
    whole = result(device, name)
    alone = forward_backward(device, name, slice(1, 2))
    assert torch.equal(alone[0], whole[0][1:2])
    assert torch.equal(alone[1], whole[1][1:2])


@pytest.mark.parametrize('name', ['first', 'odd-width', 'post'])
def test_bf16_input_returns_a_bf16_gradient(device, name):
    want = oracle.truth(name)
    leaf = want['x'].to(device, torch.bfloat16).requires_grad_(True)
    y = layer(name, leaf, want['weight'].to(device), want['bias'].to(device))
    assert y.dtype == torch.float32
    y.backward(want['upstream'].to(device))
    assert leaf.grad.dtype == torch.bfloat16 and leaf.grad.shape == leaf.shape
    exact = layer(name, leaf.detach().float(), want['weight'].to(device),
                  want['bias'].to(device))
    assert torch.equal(y, exact)


def test_autocast_computes_in_fp32(device):
    want = oracle.truth('odd-width')
    arguments = [want[k].to(device) for k in ('x', 'weight', 'bias')]
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = layer('odd-width', *arguments)
    assert y.dtype == torch.float32
    assert torch.equal(y, layer('odd-width', *arguments))


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
