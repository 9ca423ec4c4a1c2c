"""The conv stack of the multi-period discriminator on the device
(promonet_amd.model.discriminator: period_conv, period_fold_conv,
weight_norm, DiscriminatorP, Discriminator) against the float64 oracle
(tests/pconv_oracle.py) and the reference's own run (tests/golden/pconv.pt).

Gates: per quantity (forward, gx, gW, gb) 4 x the largest error that the
reference's own arithmetic in fp32 (pad, view, conv2d and leaky_relu with
autograd on the build host's CPU) shows against the same oracle over the case
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
import pconv_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.ALL_CASES)
pytestmark = pytest.mark.gpu


def layer(name, x, weight, bias):
    _, _, _, stride, slope = oracle.form_of(name)
    if name in oracle.FOLD_CASES:
        return discriminator.period_fold_conv(
            x, weight, bias, oracle.FOLD_CASES[name][1], slope)
    return discriminator.period_conv(x, weight, bias, stride, slope)


FAMILY = conv_checks.Family(
    oracle, lambda name, x, weight, bias, rows: layer(name, x, weight, bias))


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'pconv.pt')


###############################################################################
# Within the gate
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_a_layer_is_within_the_gate(device, name):
    conv_checks.a_layer_is_within_the_gate(FAMILY, device, name)


@pytest.mark.parametrize('shape', oracle.WEIGHT_NORM_SHAPES)
def test_weight_norm_is_within_the_gate(device, shape):
    """The existing weight norm at fan 5, 160, 640, 2560, 5120 and 3072"""
    conv_checks.weight_norm_is_within_the_gate(oracle, device, shape)


###############################################################################
# The modules
###############################################################################


def golden_module(golden, device, period):
    module = discriminator.DiscriminatorP(period)
    assert list(module.state_dict()) == golden['keys']
    module.load_state_dict(oracle.parameters(period))
    return module.to(device)


@pytest.mark.parametrize('period', oracle.PERIODS)
def test_the_module_gives_the_golden_within_the_gate(device, golden, period):
    module = golden_module(golden, device, period)
    audio = golden['audio'].to(device).requires_grad_(True)
    flat, maps = module(audio)
    assert len(maps) == 6 and flat.ndim == 2
    assert torch.equal(flat, torch.flatten(maps[-1], 1, -1))
    total = sum((c.to(device) * o).sum() for c, o in zip(
        oracle.golden_coefficients(golden, period), maps))
    total.backward()
    gradients = {key: value.grad.cpu()
                 for key, value in module.named_parameters()}
    figures = oracle.stack_figures(
        golden, period, maps[-1].detach().cpu(),
        [m.detach().cpu() for m in maps[:-1]], audio.grad.cpu(), gradients)
    print(' '.join(f'{label} {value:.3e}' for label, _, value in figures))
    for label, quantity, value in figures:
        assert value < oracle.gate(quantity), (label, value)


def test_the_aggregate_s_lists_are_its_members_outputs(device):
    generator = torch.Generator().manual_seed(3)
    real = .1 * torch.randn(2, 1, 4096, generator=generator).to(device)
    fake = .1 * torch.randn(2, 1, 4096, generator=generator).to(device)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        module = discriminator.Discriminator(
            (2, 11), True, [(512, 50, 240)]).to(device)
    assert [type(m).__name__ for m in module.discriminators] == [
        'DiscriminatorP', 'DiscriminatorP', 'DiscriminatorR',
        'DiscriminatorCMB']
    leaf = fake.clone().requires_grad_(True)
    lists = module(real, leaf)
    assert [len(entry) for entry in lists] == [4] * 4
    for index, member in enumerate(module.discriminators):
        for audio, logits, maps in ((real, lists[0][index], lists[2][index]),
                                    (fake, lists[1][index], lists[3][index])):
            want_logits, want_maps = member(audio)
            assert torch.equal(logits, want_logits)
            assert len(maps) == len(want_maps)
            for got, want in zip(maps, want_maps):
                assert torch.equal(got, want)
    sum(logits.sum() for logits in lists[1]).backward()
    assert leaf.grad.shape == fake.shape and leaf.grad.abs().sum() > 0.


def test_the_maps_reach_feature_matching_without_a_copy(device, golden):
    module = golden_module(golden, device, 5)
    audio = golden['audio']
    with torch.no_grad():
        real = module(audio.to(device))[1]
        fake = module((audio + .5).to(device))[1]
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


@pytest.mark.parametrize('name', NAMES)
def test_two_runs_are_bit_identical(device, name):
    conv_checks.two_runs_are_bit_identical(FAMILY, device, name)


@pytest.mark.parametrize(
    'name', ['first-2', 'second-2', 'third-2', 'fifth-large', 'post-2',
             'audio-reflect'])
def test_forward_and_backward_capture_into_one_graph(device, name):
    conv_checks.forward_and_backward_capture_into_one_graph(
        FAMILY, device, name)


@pytest.mark.parametrize(
    'name', ['first-1', 'second-2', 'fifth-2', 'post-2', 'audio-five'])
def test_zero_input_gives_the_bias(device, name):
    conv_checks.zero_input_gives_the_bias(
        FAMILY, device, name, oracle.form_of(name)[4])


@pytest.mark.parametrize(
    'name', ['first-2', 'second-2', 'third-2', 'fourth-1', 'fifth-large',
             'post-2', 'audio-reflect'])
def test_a_row_alone_equals_the_row_in_its_batch(device, name):
    conv_checks.a_row_alone_equals_the_row_in_its_batch(FAMILY, device, name)


@pytest.mark.parametrize('name', ['second-1', 'post-0', 'audio-five'])
def test_bf16_input_returns_a_bf16_gradient(device, name):
    conv_checks.bf16_input_returns_a_bf16_gradient(FAMILY, device, name)


@pytest.mark.parametrize('name', ['third-1', 'audio-five'])
def test_autocast_computes_in_fp32(device, name):
    conv_checks.autocast_computes_in_fp32(FAMILY, device, name)


def test_the_fold_equals_the_layer_on_the_folded_map(device):
    """The first layer on the audio against period_conv on the map that the
    reference's pad and view give"""
    for name in oracle.FOLD_CASES:
        want = oracle.truth(name)
        period = oracle.FOLD_CASES[name][1]
        arguments = [want[k].to(device) for k in ('weight', 'bias')]
        folded = oracle.reference_fold(want['x'], period).to(device)
        assert torch.equal(
            layer(name, want['x'].to(device), *arguments),
            discriminator.period_conv(folded, *arguments, 3, .1))
        assert torch.equal(
            layer(name, want['x'][:, 0].to(device), *arguments),
            layer(name, want['x'].to(device), *arguments))


###############################################################################
# patch(): a stand-in with the reference's layer layout
###############################################################################


def conv(*args, **kwargs):
    return torch.nn.utils.weight_norm(torch.nn.Conv2d(*args, **kwargs))


def stand_in(first_stride=(3, 1)):
    """DiscriminatorP with the reference's layer layout; a first stride of
    (1, 3) is a form the kernels do not compute"""
    calls = []

    class DiscriminatorP(torch.nn.Module):

        def __init__(self, period):
            super().__init__()
            self.period = period
            self.convs = torch.nn.ModuleList([
                conv(1, 32, (5, 1), first_stride, padding=(2, 0)),
                conv(32, 128, (5, 1), (3, 1), padding=(2, 0)),
                conv(128, 512, (5, 1), (3, 1), padding=(2, 0)),
                conv(512, 1024, (5, 1), (3, 1), padding=(2, 0)),
                conv(1024, 1024, (5, 1), 1, padding=(2, 0))])
            self.conv_post = conv(1024, 1, (3, 1), 1, padding=(1, 0))

        def forward(self, x):
            calls.append('p')
            fmap = []
            x = oracle.reference_fold(x, self.period)
            for entry in self.convs:
                x = torch.nn.functional.leaky_relu(entry(x), 0.1)
                fmap.append(x)
            x = self.conv_post(x)
            fmap.append(x)
            return torch.flatten(x, 1, -1), fmap

    return types.SimpleNamespace(DiscriminatorP=DiscriminatorP), calls


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_the_patched_module_equals_the_functions(device):
    module, calls = stand_in()
    original = module.DiscriminatorP.forward
    discriminator.patch_module(module)
    discriminator.patch_module(module)
    assert module.DiscriminatorP.forward.original is original
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        member = module.DiscriminatorP(5).to(device)
    audio = .1 * torch.randn(
        2, 1, 1023, generator=torch.Generator().manual_seed(4)).to(device)
    logits, maps = member(audio)
    assert not calls and len(maps) == 6
    first = member.convs[0]
    x = discriminator.period_fold_conv(
        audio, discriminator.weight_norm(first.weight_g, first.weight_v),
        first.bias, 5, .1)
    expected = [x]
    for entry in list(member.convs[1:]) + [member.conv_post]:
        x = discriminator.period_conv(
            x, discriminator.weight_norm(entry.weight_g, entry.weight_v),
            entry.bias, entry.stride,
            1. if entry is member.conv_post else .1)
        expected.append(x)
    assert torch.equal(logits, torch.flatten(expected[-1], 1, -1))
    for got, want in zip(maps, expected):
        assert torch.equal(got, want)
    theirs, their_maps = original(member, audio)
    assert calls == ['p']
    assert torch.allclose(logits, theirs, rtol=1e-3, atol=1e-4)
    assert [m.shape for m in maps] == [m.shape for m in their_maps]


@pytest.mark.filterwarnings('ignore::FutureWarning')
def test_a_stack_of_another_form_goes_to_the_original(device):
    module, calls = stand_in(first_stride=(1, 3))
    discriminator.patch_module(module)
    audio = .1 * torch.randn(
        2, 1, 1023, generator=torch.Generator().manual_seed(4)).to(device)
    module.DiscriminatorP(5).to(device)(audio)
    assert calls == ['p']
