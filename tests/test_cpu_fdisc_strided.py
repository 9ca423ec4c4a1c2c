"""The strided, wider layers of the FARGAN discriminator's conv stacks without
a GPU: the float64 oracle (tests/fdisc_strided_oracle.py) against torch's
conv2d and against the reference's own run at n_fft 128 ... 2048
(tests/golden/fdisc_strided.pt), the conditions the GPU tests rely on, the
planted defects their comparisons must reject, the size checks, the modules'
state_dicts and `patch()`.
"""
import types
from pathlib import Path

import pytest
import torch

from promonet_amd import _lib
from promonet_amd.model import discriminator

import conv_checks
import fdisc_strided_oracle as oracle
from conv_checks import close

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(oracle.CASES)
SIZES = (128, 256, 512, 1024, 2048)


@pytest.fixture(scope='module')
def golden():
    return torch.load(ROOT / 'tests' / 'golden' / 'fdisc_strided.pt')


@pytest.fixture(scope='module')
def recorded():
    """The reference's keys and shapes at all six sizes"""
    return torch.load(ROOT / 'tests' / 'golden' / 'fdisc.pt')


###############################################################################
# The oracle
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_layer_oracle_equals_conv2d_in_float64(name):
    _, _, _, _, stride, activation = oracle.CASES[name]
    want = oracle.truth(name)
    _, y, gradients = oracle.reference_fp32(
        want['x'], want['weight'], want['bias'], stride, activation,
        torch.float64, want['upstream'])
    assert want['forward'].shape == y.shape
    assert close(want['forward'], y)
    for quantity, theirs in zip(oracle.QUANTITIES[1:], gradients):
        assert want[quantity].shape == theirs.shape
        assert close(want[quantity], theirs), quantity


_STACKS = {}


def stack_truth(n_fft):
    """The stack of the oracle at a resolution, computed once: (logits, maps,
    gradient in x, {name: gradient})"""
    if n_fft not in _STACKS:
        parameters = oracle.listed(oracle.parameters(n_fft))
        strides = [entry[0] for entry in oracle.plan(n_fft)]
        logits, maps, saved = oracle.stack(
            oracle.stack_input(n_fft), parameters, strides)
        grad_x, gradients = oracle.stack_backward(
            saved, parameters,
            oracle.coefficients([m.shape for m in maps] + [logits.shape]))
        named = {f'layers.{i}.1.{key}': value
                 for i, triple in enumerate(gradients)
                 for key, value in zip(('weight_g', 'weight_v', 'bias'),
                                       triple)}
        _STACKS[n_fft] = logits, maps, grad_x, named
    return _STACKS[n_fft]


@pytest.mark.parametrize('n_fft', SIZES)
def test_the_stack_oracle_equals_the_reference(golden, n_fft):
    kept = golden['stacks'][n_fft]
    assert torch.equal(kept['x'], oracle.stack_input(n_fft))
    logits, maps, grad_x, named = stack_truth(n_fft)
    assert kept['logits'].dtype == torch.float64
    assert [list(m.shape) for m in maps + [logits]] == kept['shapes']
    assert close(logits, kept['logits'])
    for mine, theirs in zip(maps, kept['maps']):
        assert close(mine.flatten()[::golden['map_stride']], theirs)
    assert close(grad_x.flatten()[::golden['input_stride']],
                 kept['gradient_x'])
    assert set(named) == set(kept['gradients'])
    for key, mine in named.items():
        step = golden['gradient_stride'] if key.endswith('weight_v') else 1
        assert close(mine.flatten()[::step], kept['gradients'][key]), key


def test_the_plan_of_the_oracle_is_the_module_s():
    for n_fft in SIZES:
        assert oracle.plan(n_fft) == [
            (stride, channels, out_channels) for stride, _, channels,
            out_channels in discriminator.magfree_plan(n_fft)]
        for stride, channels, out_channels in oracle.plan(n_fft):
            narrow = stride == 1 and {channels, out_channels} <= {1, 16}
            assert narrow or (channels, out_channels, stride) in \
                discriminator.STRIDED_FORMS
    # ... and the table is no wider than the plans
    built = {(c, o, s) for n_fft in SIZES for s, c, o in oracle.plan(n_fft)}
    assert discriminator.STRIDED_FORMS <= built


###############################################################################
# What the GPU tests rely on
###############################################################################


@pytest.mark.parametrize('name', NAMES)
def test_the_fragile_share_is_small(name):
    conv_checks.the_fragile_share_is_small(oracle, name)


@pytest.mark.parametrize('name', NAMES)
def test_the_gates_come_from_the_reference_arithmetic_in_fp32(name):
    conv_checks.the_gates_come_from_the_reference_arithmetic_in_fp32(
        oracle, name)


def test_the_cases_reach_what_they_name():
    nt, kc = oracle.NT, oracle.KC
    library = _lib.lib()

    def pixels(name):
        _, _, bins, frames, stride, _ = oracle.CASES[name]
        return (oracle.BATCH * bins * frames,
                oracle.BATCH * oracle.out_bins(bins, stride) * frames)

    assert oracle.out_bins(33, 2) == 17 and oracle.out_bins(34, 2) == 17
    assert oracle.out_bins(2, 2) == 1 and oracle.out_bins(1, 2) == 1
    # the most K chunks and row blocks of the table
    assert oracle.CASES['widest'][:2] == (128, 256) and 128 // kc == 8
    # no multiple of a tile, and the first tile crosses the batch row
    total, _ = pixels('square')
    assert total % nt and total // oracle.BATCH < nt < total
    # more than one pixel tile; four gW partials of two chunks, the last of
    # one chunk whose last step of four pixels is half empty
    _, out = pixels('large')
    chunk = oracle.GW_PIX
    assert nt < out < 2 * nt
    chunks = -(-out // chunk)
    assert chunks == 7 and out % chunk == 2
    assert oracle.CONSTANTS['FS_GW_MIN_CHUNKS'] == 2
    partial = 4 * (32 * 18 * 9 + 32)
    need = library.pm_fdisc_layer_workspace_bytes(
        oracle.BATCH, 16, 32, *oracle.CASES['large'][2:4], 2)
    assert need == (4 * partial + 255) // 256 * 256
    # the edge layers: two partials
    for name, index, floats in (('first-large', 1, 16 * 27 + 16),
                                ('last-large', 0, 34 * 9 + 1)):
        walked = pixels(name)[index]
        assert oracle.EDGE < walked < 2 * oracle.EDGE
        channels, out_channels, bins, frames, stride, _ = oracle.CASES[name]
        need = library.pm_fdisc_layer_workspace_bytes(
            oracle.BATCH, channels, out_channels, bins, frames, stride)
        assert need == (2 * 4 * floats + 255) // 256 * 256
    # the narrow forms go through §21's entries
    assert library.pm_fdisc_layer_workspace_bytes(2, 16, 16, 33, 7, 1) == \
        library.pm_fdisc_workspace_bytes(2, 16, 16, 33, 7)


###############################################################################
# Planted defects: the comparisons of the GPU tests reject each of them in
# every case it can touch: the shapes and the four figures against the gates
# (test_gpu_fdisc_strided.py) and torch.equal on integers
# (test_gpu_fdisc_strided_exact.py)
###############################################################################

STRIDED = [name for name in NAMES if oracle.CASES[name][4] == 2]
ODD = [name for name in STRIDED if oracle.CASES[name][2] % 2]
EVEN = [name for name in STRIDED if not oracle.CASES[name][2] % 2]
PLAIN = [name for name in NAMES if oracle.CASES[name][4] == 1]
# a second block of FS_KC channels in the forward's K loop or in gx's
DEEP = [name for name in NAMES if max(oracle.CASES[name][:2]) >= 32]
# a second 16-row block of the forward or of gx
TALL = DEEP
WIDE = [name for name in NAMES if oracle.CASES[name][0] >= 32]
APPLIES = {
    'stride_on_time': STRIDED,
    # (at an even F the two counts agree)
    'half_bins': ODD,
    # (one bin: the angle is 0 either way)
    'angle_from_output': [name for name in STRIDED if name != 'one-bin'],
    'embedding_at_output_row': NAMES,
    'embedding_unpadded_frequency': NAMES,
    'embedding_weights_first_channels': NAMES,
    'gx_parities_exchanged': STRIDED,
    # the last input row's tap 0 has no output row: the last odd row of an
    # even F at stride 2, the last row at stride 1
    'gx_row_past_end': EVEN + PLAIN,
    'k_block_dropped': DEEP,
    'k_block_twice': DEEP,
    'row_block_overwritten': TALL,
    'gw_later_blocks_dropped': WIDE,
    'gw_embedding_dropped': NAMES,
}
# (the integer table replaces the angle)
EXACT = {defect: names for defect, names in APPLIES.items()
         if defect != 'angle_from_output'}


def accepted(name, defect):
    """Would test_gpu_fdisc_strided.py pass an implementation with this
    defect?"""
    form = oracle.CASES[name][4:]
    return conv_checks.accepted(
        oracle, name, lambda *inputs: oracle.layer(*inputs, *form, defect),
        lambda *inputs: oracle.layer_backward(*inputs, *form, defect))


def accepted_exactly(name, defect):
    """Would test_gpu_fdisc_strided_exact.py?"""
    for which in ('x', 'table'):
        x, weight, bias, upstream, table, stride, activation = \
            oracle.integer_case(name, which)
        y = oracle.layer(x, weight, bias, stride, activation, table=table)
        want = (y,) + oracle.layer_backward(
            x, weight, y, upstream, stride, activation, table=table)
        mine = oracle.layer(
            x, weight, bias, stride, activation, defect, table)
        if mine.shape != y.shape:
            return False
        got = (mine,) + oracle.layer_backward(
            x, weight, mine, upstream, stride, activation, defect, table)
        for label, a, b in zip(oracle.QUANTITIES, got, want):
            if label == 'gW' and which == 'x':
                a, b = a[:, :x.shape[1]], b[:, :x.shape[1]]
            if not torch.equal(a, b):
                return False
    return True


def test_the_defects_are_all_listed():
    assert set(APPLIES) == set(oracle.DEFECTS)
    assert all(APPLIES.values())


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_itself_is_accepted(name):
    assert accepted(name, None) and accepted_exactly(name, None)


@pytest.mark.parametrize(
    'defect,name',
    [(defect, name) for defect in APPLIES for name in APPLIES[defect]])
def test_a_planted_defect_is_rejected_by_the_gates(defect, name):
    assert not accepted(name, defect)


@pytest.mark.parametrize(
    'defect,name',
    [(defect, name) for defect in EXACT for name in EXACT[defect]])
def test_a_planted_defect_is_rejected_by_the_integers(defect, name):
    assert not accepted_exactly(name, defect)


@pytest.mark.parametrize('which', ['x', 'table'])
@pytest.mark.parametrize('name', NAMES)
def test_the_integer_sums_are_exact_in_fp32(name, which):
    """Every partial sum is an integer below 2^24: at most 258 x 9 products
    of at most 16 a pre-activation, and the sums over the pixels stay there"""
    x, weight, bias, upstream, table, stride, activation = \
        oracle.integer_case(name, which)
    y = oracle.layer(x, weight, bias, stride, activation, table=table)
    want = (y,) + oracle.layer_backward(
        x, weight, y, upstream, stride, activation, table=table)
    if which == 'x':
        # (the weight gradient of the embedding channels is a sum of sines:
        # it is exact under the integer table)
        want = want[:2] + (want[2][:, :x.shape[1]],) + want[3:]
    assert all(v.abs().max() < 2 ** 24 and torch.equal(v, v.round())
               for v in want)
    # the sum of the magnitudes bounds every partial sum in any order: the
    # products are at most 16, a pre-activation or an input gradient has at
    # most 258 x 9 of them, a weight gradient one a pixel
    assert 258 * 9 * 16 < 2 ** 24
    assert upstream[:, 0].numel() * 16 < 2 ** 24
    if activation == 'relu':
        assert (y > 0).any() and (y == 0).any()


###############################################################################
# Sizes: ValueError from Python, PM_EINVAL from the ABI, no device needed
###############################################################################

ABI_BAD = [
    # batch, channels, out_channels, bins, frames, stride, activation
    (2, 8, 16, 33, 7, 1, 1),
    (2, 16, 64, 33, 7, 1, 1),           # a form outside the table
    (2, 32, 32, 33, 7, 2, 1),
    (2, 16, 16, 33, 7, 2, 1),
    (2, 256, 256, 33, 7, 1, 1),
    (2, 16, 1, 33, 7, 2, 1),
    (2, 1, 1, 33, 7, 1, 1),
    (2, 512, 1, 33, 7, 1, 1),
    (2, 32, 64, 33, 7, 3, 1),           # the stride
    (2, 32, 64, 33, 7, 0, 1),
    (0, 32, 64, 33, 7, 2, 1),
    (2, 32, 64, 0, 7, 2, 1),
    (2, 32, 64, 33, 0, 2, 1),
    (2, 32, 64, 33, 7, 2, 3),
    (2, 32, 64, 33, 7, 2, -1),
    (1 << 20, 32, 64, 1 << 10, 1 << 10, 2, 1),      # 2^40 pixels
    (1 << 11, 32, 64, 1 << 10, 1 << 10, 2, 1),      # 2^31 input pixels
]


@pytest.mark.parametrize('sizes', ABI_BAD)
def test_the_abi_refuses_bad_sizes_on_the_host(sizes):
    library = _lib.lib()
    if 0 <= sizes[6] < 3:
        assert library.pm_fdisc_layer_workspace_bytes(*sizes[:6]) == 0
    # (the pointers are never read: the sizes are refused first)
    code = library.pm_fdisc_layer_forward(
        256, 256, 256, 256, 256, *sizes, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_layer_forward' in library.pm_last_error()
    code = library.pm_fdisc_layer_backward(
        256, 256, 256, 256, 256, 256, 256, 256, *sizes, 256, 1 << 40, None)
    assert code == _lib.PM_EINVAL
    assert b'pm_fdisc_layer_backward' in library.pm_last_error()


@pytest.mark.parametrize('form', sorted(discriminator.STRIDED_FORMS) +
                         [(1, 16, 1), (16, 16, 1), (16, 1, 1)])
def test_the_abi_accepts_every_form_of_the_table(form):
    channels, out_channels, stride = form
    need = _lib.lib().pm_fdisc_layer_workspace_bytes(
        2, channels, out_channels, 9, 5, stride)
    assert need >= 256 and need % 256 == 0


def test_the_abi_refuses_null_pointers_and_a_small_workspace():
    library = _lib.lib()
    for sizes in ((2, 32, 64, 33, 7, 2, 1), (2, 16, 16, 33, 7, 1, 1),
                  (2, 1, 16, 33, 7, 2, 1), (2, 64, 1, 33, 7, 1, 2)):
        need = library.pm_fdisc_layer_workspace_bytes(*sizes[:6])
        assert need >= 256 and need % 256 == 0
        code = library.pm_fdisc_layer_forward(
            256, 256, None, 256, 256, *sizes, None)
        assert code == _lib.PM_EINVAL
        assert b'pm_fdisc_layer_forward' in library.pm_last_error()
        code = library.pm_fdisc_layer_backward(
            256, 256, 256, 256, 256, 256, 256, None, *sizes, 256, need, None)
        assert code == _lib.PM_EINVAL
        assert b'pm_fdisc_layer_backward' in library.pm_last_error()
        code = library.pm_fdisc_layer_backward(
            256, 256, 256, 256, 256, 256, 256, 256, *sizes, 256, need - 1,
            None)
        assert code == _lib.PM_ENOMEM
        assert b'pm_fdisc_layer_backward' in library.pm_last_error()


def arguments(channels=32, out_channels=64, bins=9, frames=5):
    return (torch.zeros(2, channels, bins, frames),
            torch.zeros(out_channels, channels + 2, 3, 3),
            torch.zeros(out_channels))


@pytest.mark.parametrize('form', [
    (16, 64, 1), (32, 32, 2), (16, 16, 2), (256, 256, 1), (16, 1, 2),
    (8, 8, 1), (48, 96, 2), (512, 1, 1)])
def test_a_form_outside_the_table_raises_before_any_device_work(form):
    channels, out_channels, stride = form
    with pytest.raises(ValueError):
        discriminator.frequency_conv(
            *arguments(channels, out_channels), stride=stride)


@pytest.mark.parametrize('keywords', [
    {'stride': 2, 'dilation': 2}, {'stride': 1, 'dilation': 2},
    {'stride': 2, 'dilation': (1, 2)}, {'stride': 3}, {'stride': 0},
    {'stride': True}, {'stride': 2, 'activation': 'tanh'},
    {'stride': 2, 'table': torch.zeros(5, 2)}])
def test_bad_keywords_raise_before_any_device_work(keywords):
    with pytest.raises(ValueError):
        discriminator.frequency_conv(*arguments(), **keywords)


def test_good_sizes_on_a_cpu_tensor_say_that_there_is_no_fallback():
    for keywords in ({'stride': 2}, {'stride': 1}, {'dilation': (1, 1)}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            discriminator.frequency_conv(*arguments(), **keywords)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        discriminator.frequency_conv(*arguments(256, 1), activation='sigmoid')


###############################################################################
# The modules
###############################################################################


@pytest.mark.parametrize('n_fft', discriminator.RESOLUTIONS)
def test_the_strided_module_has_the_reference_s_keys_and_shapes(
        recorded, n_fft):
    module = discriminator.DiscriminatorMagFree(
        [n_fft, n_fft // 4, n_fft], strided=True)
    state = module.state_dict()
    assert list(state) == recorded['keys'][n_fft]
    assert [list(v.shape) for v in state.values()] == recorded['shapes'][n_fft]
    assert not module.filterbank.requires_grad
    assert [layer[1].stride for layer in module.layers] == [
        entry[0][0] for entry in recorded['plans'][n_fft]]
    if n_fft > 64:
        # the hashed parameters load
        kept = oracle.parameters(n_fft)
        module.load_state_dict(
            dict(kept, filterbank=torch.ones_like(state['filterbank'])))
        assert torch.equal(module.layers[4][1].weight_v,
                           kept['layers.4.1.weight_v'])


@pytest.mark.parametrize('n_fft', discriminator.RESOLUTIONS[1:])
def test_the_default_still_refuses_and_names_the_keyword(n_fft):
    with pytest.raises(ValueError, match='strided=True'):
        discriminator.DiscriminatorMagFree([n_fft, n_fft // 4, n_fft])


def test_the_aggregate_has_the_keys_of_the_fargan_configuration(recorded):
    """config/fargan-fdisc.py: FARGAN_DISCRIMINATOR alone, the period and the
    complex multi-band members switched off (the scale and the resolution
    members are off by default)"""
    module = discriminator.Discriminator(
        periods=(), complex_multiband=False,
        fargan=discriminator.RESOLUTIONS)
    state = module.state_dict()
    keys, shapes = [], []
    for index, n_fft in enumerate(discriminator.RESOLUTIONS):
        keys += [f'discriminators.{index}.{key}'
                 for key in recorded['keys'][n_fft]]
        shapes += recorded['shapes'][n_fft]
    assert list(state) == keys
    assert [list(v.shape) for v in state.values()] == shapes
    assert [member.resolution for member in module.discriminators] == [
        (n, n // 4, n) for n in discriminator.RESOLUTIONS]
    # a state_dict of that shape loads with strict=True
    module.load_state_dict(
        {key: torch.full_like(value, .5) for key, value in state.items()},
        strict=True)
    # ... after the reference's other members, in its order
    both = discriminator.Discriminator(periods=(2,), fargan=(128,))
    assert [type(member).__name__ for member in both.discriminators] == [
        'DiscriminatorP', 'DiscriminatorCMB', 'DiscriminatorMagFree']


###############################################################################
# patch(): which stacks take the device path
###############################################################################


class FrequencyPositionalEmbedding(torch.nn.Identity):
    pass


def reference_layers(n_fft, change=None):
    """self.layers in the reference's layout at a resolution; `change`
    (index, keywords) rebuilds one conv otherwise"""
    layers = []
    for index, (stride, dilation, channels, out_channels) in enumerate(
            discriminator.magfree_plan(n_fft)):
        keywords = dict(stride=(stride, 1), dilation=(dilation, 1),
                        padding=(dilation, 1))
        if change is not None and change[0] == index:
            keywords.update(change[1])
        layers.append(torch.nn.Sequential(
            FrequencyPositionalEmbedding(),
            torch.nn.utils.weight_norm(torch.nn.Conv2d(
                channels + 2, out_channels, (3, 3), **keywords)),
            torch.nn.Sigmoid() if index == 5 else torch.nn.ReLU()))
    return types.SimpleNamespace(layers=torch.nn.ModuleList(layers))


@pytest.mark.parametrize('n_fft', discriminator.RESOLUTIONS)
def test_the_reference_s_stacks_take_the_device_path(n_fft):
    found = discriminator._stack_layers(reference_layers(n_fft))
    assert [(entry[1], entry[3]) for entry in found] == [
        (dilation, stride) for stride, dilation, _, _ in
        discriminator.magfree_plan(n_fft)]


@pytest.mark.parametrize('change', [
    (1, dict(stride=(2, 2))),                   # a stride on the time axis
    (1, dict(dilation=(2, 1), padding=(2, 1))),     # a strided layer, dilated
    (1, dict(padding=(0, 1))),
    (3, dict(stride=(2, 1))),                   # 64 -> 64 at stride 2
])
def test_a_stack_with_another_layer_goes_to_the_original(change):
    assert discriminator._stack_layers(reference_layers(256, change)) is None
