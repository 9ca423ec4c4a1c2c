"""The case table of tests/nonfinite_oracle.py stands on its own: the clean
truths are finite, a plant arrives where it must and nowhere else, the BAD
masks of the conv layer and of the transforms are the receptive field that the
case's geometry gives (so no mask rests on a padding convention), every
element of another batch row is CLEAN, the two gradients with two outcomes
have one of them, and the oracles' elementwise ops on non-finite values are torch's own
with autograd."""
import pytest
import torch

from promonet_amd import _lib

import adversarial_oracle
import disc_spectrogram_oracle
import fdisc_oracle
import fdisc_strided_oracle
import losses_oracle
import nonfinite_oracle as oracle

NAN, INF = oracle.NAN, oracle.INF
VALUE_IDS = list(oracle.VALUES)


def sets(clean, planted, key):
    return oracle.masks(clean[key], planted[key])


def assert_finite(outputs):
    for key, tensor in outputs.items():
        assert torch.isfinite(tensor).all(), key


###############################################################################
# The multi-tensor mean
###############################################################################


@pytest.mark.parametrize('dtype', list(oracle.ADV_DTYPES))
@pytest.mark.parametrize('op', adversarial_oracle.OPS)
def test_multi_mean(op, dtype):
    chunk = _lib.lib().pm_multi_mean_chunk()
    kind = oracle.ADV_DTYPES[dtype]
    assert oracle.adversarial_sizes(chunk) == (1, chunk - 1, chunk + 3)
    sites = oracle.adversarial_plants(op, chunk)
    assert ('b', 2, chunk + 1) in sites or op != adversarial_oracle.ABS_DIFF
    for site in sites:
        for value in oracle.VALUES.values():
            (a, b), clean, _, planted = oracle.adversarial_case(
                op, kind, chunk, site, value)
            assert_finite(clean)
            # (no exact zero: a Gaussian in 16 bits has none either)
            assert all((t != 0).all() for t in a)
            _, index, element = site
            means = sets(clean, planted, 'means')
            touched = torch.zeros(3, dtype=torch.bool)
            touched[index] = True
            # (a hinge closes on the infinity of its own side: max(1 - inf,
            # 0) = 0 is finite, and the mean only changes)
            closes = (op, value) in (
                (adversarial_oracle.HINGE_ONE_MINUS, INF),
                (adversarial_oracle.HINGE_ONE_PLUS, -INF))
            assert torch.equal(means['bad'], touched & (not closes))
            assert means['clean'][~touched].all()
            assert sets(clean, planted, 'total')['bad'].all() != closes
            for k in range(3):
                gradient = sets(clean, planted, f'gradient{k}')
                elsewhere = torch.ones_like(gradient['clean'])
                if k == index:
                    elsewhere[element] = False
                assert gradient['clean'][elsewhere].all()


@pytest.mark.parametrize('op', adversarial_oracle.OPS)
def test_the_terms_are_torch_s(op):
    """term / derivative on non-finite values against the reference's formula
    through autograd"""
    a = torch.tensor([NAN, INF, -INF, 1., -1., .5, -3.], dtype=torch.float64)
    b = torch.tensor([.5, .5, .5, NAN, INF, -INF, 2.], dtype=torch.float64)
    leaf_a, leaf_b = (t.clone().requires_grad_(True) for t in (a, b))
    theirs = {
        adversarial_oracle.ABS_DIFF: lambda: torch.abs(leaf_a - leaf_b),
        adversarial_oracle.SQ_ONE_MINUS: lambda: (1. - leaf_a) ** 2.,
        adversarial_oracle.SQ: lambda: leaf_a ** 2.,
        adversarial_oracle.HINGE_ONE_MINUS:
            lambda: torch.clamp(1. - leaf_a, min=0.),
        adversarial_oracle.HINGE_ONE_PLUS:
            lambda: torch.clamp(1. + leaf_a, min=0.)}[op]()
    theirs.sum().backward()
    other = b if op == adversarial_oracle.ABS_DIFF else None
    assert torch.equal(adversarial_oracle.term(op, a, other).nan_to_num(7.),
                       theirs.detach().nan_to_num(7.))
    gradient = leaf_b.grad if op == adversarial_oracle.ABS_DIFF \
        else leaf_a.grad
    ours = adversarial_oracle.derivative(op, a, other)
    assert torch.equal(torch.isfinite(ours), torch.isfinite(gradient))
    assert torch.equal(ours.nan_to_num(7.), gradient.nan_to_num(7.))
    if op in (adversarial_oracle.HINGE_ONE_MINUS,
              adversarial_oracle.HINGE_ONE_PLUS):
        # the hinge of a NaN is NaN, and its derivative 0
        assert torch.isnan(theirs[0]) and gradient[0] == 0.


###############################################################################
# The frequency conv layer
###############################################################################


def channels_of(field, channels):
    """(B, F, T) -> (B, channels, F, T)"""
    return field[:, None].expand(-1, channels, -1, -1)


def links(bins_out, frames, pairs, t):
    """[(kf, kt, output row, output frame)] of the taps that read an input
    pixel of frame t, `pairs` its (kf, output row), inside the output map"""
    return [(kf, kt, row, t + 1 - kt) for kf, row in pairs for kt in range(3)
            if 0 <= row < bins_out and 0 <= t + 1 - kt < frames]


def input_plant_masks(weight, index, value, linked, shape, relu):
    """From the geometry and the sign of w * value alone: the BAD mask of the
    forward (a ReLU keeps +inf and turns -inf into 0; a NaN stays) and of gW
    (the plant's channel at every linked tap, every output channel: gz times
    the plant is non-finite even where gz is 0)"""
    row, channel = index[:2]
    forward = torch.zeros(shape, dtype=torch.bool)
    gw = torch.zeros(weight.shape, dtype=torch.bool)
    for kf, kt, f, t in linked:
        gw[:, channel, kf, kt] = True
        product = weight[:, channel, kf, kt].double() * value
        forward[row, :, f, t] = torch.isnan(product) | (product > 0.) \
            if relu else torch.isnan(product)
    return forward, gw


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('site', ['x-last-pixel', 'x-inside',
                                  'upstream-inside'])
@pytest.mark.parametrize('name', oracle.FDISC_CASES)
def test_frequency_conv(name, site, value):
    channels, out_channels, bins, frames, _, activation = \
        fdisc_oracle.CASES[name]
    where, index = oracle.fdisc_sites(name)[site]
    tensors, clean, _, planted = oracle.fdisc_case(
        name, site, oracle.VALUES[value])
    assert_finite(clean)
    assert (tensors['x'] != 0).all()
    field = oracle.fdisc_field(name, index)
    row = index[0]
    assert field[row].any() and not field[1 - row].any()
    forward, gx = (sets(clean, planted, key) for key in ('forward', 'gx'))
    gw, gb = (sets(clean, planted, key) for key in ('gW', 'gb'))
    # the other batch row does not hear of it
    assert forward['clean'][1 - row].all() and gx['clean'][1 - row].all()
    if where == 'x':
        # forward: every output channel of the pixels a tap links to the plant
        reached = channels_of(field, out_channels)
        assert forward['clean'][~reached].all()
        if value == 'nan':
            assert torch.equal(forward['bad'], reached)
        else:
            # (w * inf is +inf or -inf: a ReLU turns one of them into 0, the
            # sigmoid both into 0 or 1)
            assert not forward['clean'][reached].all()
        dilation = fdisc_oracle.CASES[name][4]
        linked = links(bins, frames, [
            (kf, index[2] - (kf - 1) * dilation) for kf in range(3)],
            index[3])
        want_forward, want_gw = input_plant_masks(
            tensors['weight'], index, oracle.VALUES[value], linked,
            forward['bad'].shape, activation == 'relu')
        assert torch.equal(forward['bad'], want_forward)
        if activation == 'sigmoid' and value == 'nan':
            # y (1 - y) of a NaN output: every sum over the pixels has it
            assert gw['bad'].all() and gb['bad'].all()
            return
        # gW: the plant's input channel, at the taps that stay in the map
        assert torch.equal(gw['bad'], want_gw)
    else:
        # an interior upstream plant behind an open gate: the whole field in
        # gx, its output channel in gW (every tap, every input channel) and gb
        assert int(field.sum()) == 9
        assert forward['clean'].all()
        assert torch.equal(gx['bad'], channels_of(field, channels))
        expected = torch.zeros_like(gw['bad'])
        expected[index[1]] = True
        assert torch.equal(gw['bad'], expected)
        assert torch.equal(gb['bad'], expected[:, 0, 0, 0])
        assert gx['clean'][~gx['bad']].all()
        assert gw['clean'][~gw['bad']].all() and gb['clean'][~gb['bad']].all()


def test_the_activations_are_torch_s():
    z = torch.tensor([NAN, INF, -INF, 2., -2., 3., -3.], dtype=torch.float64)
    upstream = torch.tensor([1., 1., 1., INF, INF, NAN, NAN],
                            dtype=torch.float64)
    for activation, function in (('relu', torch.relu),
                                 ('sigmoid', torch.sigmoid)):
        leaf = z.clone().requires_grad_(True)
        theirs = function(leaf)
        theirs.backward(upstream)
        y = fdisc_oracle.activate(z, activation)
        assert torch.equal(y.nan_to_num(7.), theirs.detach().nan_to_num(7.))
        # the gate of layer_backward, read off its bias gradient: one pixel a
        # channel
        shape = (1, z.numel(), 1, 1)
        _, _, gate = fdisc_oracle.layer_backward(
            torch.zeros(1, 1, 1, 1), torch.zeros(z.numel(), 3, 3, 3),
            y.reshape(shape), upstream.reshape(shape), 1, activation)
        assert torch.equal(torch.isfinite(gate), torch.isfinite(leaf.grad))
        assert torch.allclose(gate.nan_to_num(7.), leaf.grad.nan_to_num(7.),
                              rtol=1e-15, atol=0.)
    # relu(NaN) is NaN and passes its gradient; a closed gate stops an inf
    leaf = z.clone().requires_grad_(True)
    torch.relu(leaf).backward(upstream)
    assert leaf.grad[0] == 1. and leaf.grad[4] == 0.


###############################################################################
# The strided frequency conv layer
###############################################################################

STRIDED_PLANTS = [(name, site) for name in oracle.STRIDED_CASES
                  for site in oracle.strided_sites(name)]


def test_the_strided_plants():
    """Every case has both input plants, and the upstream plant wherever a
    pixel of the output has all its taps inside the input"""
    missing = [(name, site) for name in oracle.STRIDED_CASES
               for site in ('x-last-pixel', 'x-inside', 'upstream-inside')
               if (name, site) not in STRIDED_PLANTS]
    assert missing == [('two-bins', 'upstream-inside')]
    # (two bins: one output row, whose taps kf = 0 lie above the map)
    assert fdisc_strided_oracle.CASES['two-bins'][2] == 2


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('name,site', STRIDED_PLANTS)
def test_strided_frequency_conv(name, site, value):
    channels, out_channels, bins, frames, stride, activation = \
        fdisc_strided_oracle.CASES[name]
    where, index = oracle.strided_sites(name)[site]
    tensors, clean, _, planted = oracle.strided_case(
        name, site, oracle.VALUES[value])
    assert_finite(clean)
    assert (tensors['x'] != 0).all()
    field, whole = oracle.strided_fields(name, index, where == 'upstream')
    row = index[0]
    assert field[row].any() and not field[1 - row].any()
    forward, gx = (sets(clean, planted, key) for key in ('forward', 'gx'))
    gw, gb = (sets(clean, planted, key) for key in ('gW', 'gb'))
    assert forward['clean'][1 - row].all() and gx['clean'][1 - row].all()
    if where == 'x':
        reached = channels_of(field, out_channels)
        assert forward['clean'][~reached].all()
        if value == 'nan':
            assert torch.equal(forward['bad'], reached)
        else:
            assert not forward['clean'][reached].all()
        linked = links(
            fdisc_strided_oracle.out_bins(bins, stride), frames,
            fdisc_strided_oracle.reaching(index[2], stride), index[3])
        want_forward, want_gw = input_plant_masks(
            tensors['weight'], index, oracle.VALUES[value], linked,
            forward['bad'].shape, activation == 'relu')
        assert torch.equal(forward['bad'], want_forward)
        if activation == 'sigmoid' and value == 'nan':
            assert gw['bad'].all() and gb['bad'].all()
            return
        assert torch.equal(gw['bad'], want_gw)
    else:
        assert whole and int(field.sum()) == 9
        assert forward['clean'].all()
        assert torch.equal(gx['bad'], channels_of(field, channels))
        expected = torch.zeros_like(gw['bad'])
        expected[index[1]] = True
        assert torch.equal(gw['bad'], expected)
        assert torch.equal(gb['bad'], expected[:, 0, 0, 0])
        assert gx['clean'][~gx['bad']].all()
        assert gw['clean'][~gw['bad']].all() and gb['clean'][~gb['bad']].all()


###############################################################################
# Weight norm
###############################################################################


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('site', list(oracle.WEIGHT_NORM_SITES))
def test_weight_norm(site, value):
    """The norm is per output channel: the plant's channel and no other"""
    assert oracle.WEIGHT_NORM_SHAPE == (16, 18, 3, 3)
    where, index = oracle.WEIGHT_NORM_SITES[site]
    tensors, clean, _, planted = oracle.weight_norm_case(
        site, oracle.VALUES[value])
    assert_finite(clean)
    assert (tensors['v'] != 0).all()
    row = torch.zeros(16, dtype=torch.bool)
    row[index[0]] = True
    forward = sets(clean, planted, 'forward')
    g_g, g_v = sets(clean, planted, 'g_g'), sets(clean, planted, 'g_v')
    assert forward['clean'][~row].all() and g_v['clean'][~row].all()
    assert torch.equal(g_g['bad'].reshape(-1), row)
    assert torch.equal(g_v['bad'].flatten(1).all(1), row)
    if where == 'upstream':
        assert forward['clean'].all()
    elif value == 'nan':
        assert torch.equal(forward['bad'].flatten(1).all(1), row)
    else:
        # v / |v| with |v| = inf: 0 but at the plant, inf / inf
        expected = torch.zeros_like(forward['bad'])
        expected[index] = True
        assert torch.equal(forward['bad'], expected)
        assert (planted['forward'][index[0]][~expected[index[0]]] == 0.).all()


###############################################################################
# The discriminator spectrograms
###############################################################################


def frame_mask(name, shape, frames, row):
    """The elements of `frames` of batch row `row` in the output's layout"""
    kind = disc_spectrogram_oracle.CASES[name][0]
    out = torch.zeros(shape, dtype=torch.bool)
    for frame in frames:
        if kind == 'R':
            out[row, :, :, frame] = True
        elif kind == 'CMB':
            out[row, :, frame, :] = True
        else:
            out[row, :, frame] = True
    return out


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('site', ['x-inside', 'x-last-sample',
                                  'upstream-inside'])
@pytest.mark.parametrize('name', oracle.SPECTROGRAM_CASES)
def test_spectrogram(name, site, value):
    kind = disc_spectrogram_oracle.CASES[name][0]
    where, index = oracle.spectrogram_sites(name)[site]
    tensors, clean, _, planted = oracle.spectrogram_case(
        name, site, oracle.VALUES[value])
    assert_finite(clean)
    assert (tensors['x'] != 0).all() and index[0] == 0
    geometry = oracle.spectrogram_geometry(name)
    free = oracle.two_outcomes('spectrogram', name, where, oracle.VALUES[value])
    assert free == (('gx',) if kind == 'DB' and where == 'x'
                    and value != 'nan' else ())
    for key in free:
        assert oracle.is_one_of_the_two(planted[key])
    forward, gx = sets(clean, planted, 'forward'), sets(clean, planted, 'gx')
    assert not forward['changed'].any()
    if where == 'x':
        frames = oracle.frames_of(index[1], *geometry)
        assert frames
        if site == 'x-last-sample':
            # (read by the last frame through the right margin alone)
            assert geometry[4] - 1 in frames
        if kind == 'DB':
            # one maximum and one floor for the whole batch
            assert forward['bad'].all()
            if not free:
                assert gx['bad'].all()
            return
        assert torch.equal(forward['bad'], frame_mask(
            name, forward['bad'].shape, frames, 0))
        covered = torch.zeros(geometry[0], dtype=torch.bool)
        for frame in frames:
            covered |= oracle.samples_of(frame, *geometry[:4])
        assert torch.equal(gx['bad'][0], covered)
    else:
        assert forward['clean'].all()
        frame = index[{'R': 3, 'CMB': 2, 'DB': 2}[kind]]
        assert 0 < frame < geometry[4] - 1
        assert torch.equal(
            gx['bad'][0], oracle.samples_of(frame, *geometry[:4]))
    assert not gx['changed'].any()
    assert gx['clean'][1].all() and forward['clean'][1].all()


def test_the_decibel_ops_are_torch_s():
    """amplitude_to_db is torch.clamp, amax and maximum: one NaN makes all of
    it NaN, and the gradient wherever the clamp passes one"""
    x = torch.tensor([[1., NAN, 3.], [1e-7, 2., .5]], dtype=torch.float64)
    leaf = x.clone().requires_grad_(True)
    out = disc_spectrogram_oracle.amplitude_to_db(leaf)
    assert torch.isnan(out).all()
    out.backward(torch.ones_like(out))
    # (wherever the clamp passes a gradient: not under 1e-5, nor at the NaN)
    assert torch.equal(torch.isnan(leaf.grad), x >= 1e-5)
    assert (leaf.grad[~(x >= 1e-5)] == 0.).all()
    db = 20. * torch.log10(torch.clamp(x, min=1e-5))
    assert torch.isnan(torch.maximum(db, db.amax() - 80.)).all()
    assert torch.isnan(torch.clamp(x, min=1e-5)[0, 1])


###############################################################################
# loss.stft, SpectralConvergence, loss.signal
###############################################################################

LOSS_PLANTS = [(entry, site) for entry in oracle.LOSS_ENTRIES
               for site in oracle.loss_sites(entry)]


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('entry,site', LOSS_PLANTS)
def test_loss(entry, site, value):
    assert oracle.LOSS_SIZES == (64, 16, 64)
    assert oracle.LOSS_SHAPE in losses_oracle.SHAPES
    where, index = oracle.loss_sites(entry)[site]
    tensors, clean, _, planted = oracle.loss_case(
        entry, site, oracle.VALUES[value])
    assert_finite(clean)
    assert (tensors['x'] != 0).all() and (tensors['y'] != 0).all()
    assert index[0] == 0
    free = oracle.two_outcomes('loss', entry, where, oracle.VALUES[value])
    assert free == (('gx',) if entry == 'spectral_convergence'
                    and where == 'y' and value != 'nan' else ())
    for key in free:
        assert oracle.is_one_of_the_two(planted[key])
    geometry = oracle.loss_geometry()
    forward, gx = sets(clean, planted, 'forward'), sets(clean, planted, 'gx')
    assert not forward['changed'].any()
    if not free:
        assert not gx['changed'].any()
    if entry == 'signal':
        # the row's norm: the whole row, and the mean over the rows
        assert forward['bad'].all()
        assert gx['bad'][0].all() and gx['clean'][1].all()
        return
    if where == 'upstream':
        assert forward['clean'].all()
        assert torch.equal(
            gx['bad'][0], oracle.samples_of(index[2], *geometry[:4]))
        assert gx['clean'][1].all()
        return
    if entry == 'spectral_convergence':
        assert forward['bad'].all()
        if where == 'y':
            # sum s_y divides every element
            assert free or gx['bad'].all()
            return
    frames = oracle.frames_of(index[1], *geometry)
    assert frames
    covered = torch.zeros(geometry[0], dtype=torch.bool)
    for frame in frames:
        covered |= oracle.samples_of(frame, *geometry[:4])
    assert torch.equal(gx['bad'][0], covered) and gx['clean'][1].all()
    if entry == 'stft':
        expected = torch.zeros_like(forward['bad'])
        expected[0][:, frames] = True
        assert torch.equal(forward['bad'], expected)


def test_the_magnitude_root_is_torch_s():
    x = torch.tensor([NAN, INF, 1e-9, 4.], dtype=torch.float64)
    ours = losses_oracle.magnitude_root(x.to(torch.complex128))
    theirs = torch.sqrt(torch.clamp(x, min=1e-7))
    assert torch.equal(ours.nan_to_num(7.), theirs.nan_to_num(7.))
    assert torch.isnan(ours[0]) and torch.isinf(ours[1])


def test_the_embedding_table_is_the_oracle_s_in_fp32():
    """The truths of the conv layers read sin and cos at fp32's values (as
    the device's table and the reference in fp32 hold them): half an fp32 ulp
    of the argument, 2 pi 2^-24, from the float64 embedding, and not tiny
    where float64's is (sin pi)"""
    for bins in (2, 33, 34, 70):
        table = oracle.embedding_table(bins).double()
        sin, cos = fdisc_oracle.embedding(bins)
        assert (table - torch.stack((sin, cos), 1)).abs().max() < 1e-6
    assert oracle.embedding_table(34)[17, 0].abs() > 1e-8
    assert fdisc_oracle.embedding(34)[0][17].abs() < 1e-15
