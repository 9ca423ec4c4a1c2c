"""The training kernels on inf and NaN against tests/nonfinite_oracle.py: an
overflowed activation or gradient must stay non-finite, where torch's ops
keep it so, until it reaches the optimizer, and must touch nothing else.

For every case and plant the device runs the clean and the planted inputs
through the public entries, and every output is held to three things
(`compare`):
  1. not isfinite(got) == BAD, exactly (inf against NaN is not told apart);
  2. on CLEAN the planted run has the bits of the clean run (the order of a
     sum does not depend on its values: no tolerance exists). This is what
     catches a halo, a padded channel, a ragged tail or a neighbouring batch
     row that is kept out by a multiplication with zero;
  3. on CHANGED the error against the planted truth, relative to the RMS of
     the clean truth, is within the family's existing gate (fdisc_oracle.gate
     and WEIGHT_NORM_GATES; the 2^-24 model of test_gpu_adversarial.py). The
     spectrogram and loss plants have no CHANGED element (test_cpu_nonfinite.py asserts it).

The stack test ties it to the scaler: a DiscriminatorMagFree on audio with one
non-finite sample, loss.discriminator (and, as the generator's step,
loss.generator with loss.feature_matching on the maps), backward, the
optimizer's statistics pass and GradScaler.step.
"""
import pytest
import torch

import promonet_amd
from promonet_amd import _lib, loss, optim
from promonet_amd.model import discriminator

import adversarial_oracle
import disc_spectrogram_oracle
import fdisc_oracle
import fdisc_strided_oracle
import nonfinite_oracle as oracle
from util import check

pytestmark = pytest.mark.gpu
VALUE_IDS = list(oracle.VALUES)
# test_gpu_adversarial.py: GAUSSIAN_GATE, in units of 2^-24 relative
ADVERSARIAL_GATE = 7.97 * oracle.EPS


def bits(tensor):
    return tensor.contiguous().view(
        torch.int32 if tensor.element_size() == 4 else torch.int16)


def compare(kind, got_clean, got_planted, clean, planted, gate, either=()):
    """The three assertions on every output; an output of `either` is held
    to being one of its two outcomes, whole (oracle.two_outcomes). Every miss
    of a case is listed before the test fails"""
    misses = []
    assert set(got_planted) == set(planted)
    for key, want in planted.items():
        if key in either:
            if not oracle.is_one_of_the_two(got_planted[key].cpu()):
                misses.append(f'{key}: neither all BAD nor all zero')
            continue
        sets = oracle.masks(clean[key], want)
        before = got_clean[key].cpu().reshape(want.shape)
        after = got_planted[key].cpu().reshape(want.shape)
        bad = ~torch.isfinite(after.float())
        if not torch.equal(bad, sets['bad']):
            misses.append(
                f'{key}: BAD {int(sets["bad"].sum())} in the truth, '
                f'{int(bad.sum())} on the device, '
                f'{int((bad ^ sets["bad"]).sum())} differ')
        same = sets['clean']
        if not torch.equal(bits(after)[same], bits(before)[same]):
            moved = int((bits(after) != bits(before))[same].sum())
            misses.append(f'{key}: {moved} CLEAN elements changed their bits')
        which = sets['changed'] & ~bad
        if which.any():
            assert gate is not None, (kind, key, 'CHANGED is not empty')
            # (a 16-bit output: the truth rounded once to the output's format)
            target = want if after.dtype == torch.float32 \
                else want.to(after.dtype)
            error = (after.double() - target.double())[which].abs().max()
            figure = (error / clean[key].double().pow(2).mean().sqrt()).item()
            limit = gate(key) if callable(gate) else gate
            print(f'{kind} {key}: CHANGED {int(which.sum())} elements, '
                  f'{figure:.3e} (gate {limit:.3e})')
            try:
                check(figure, limit, f'nonfinite/{kind.split()[0]}/{key}')
            except AssertionError as error:
                misses.append(f'{key}: CHANGED {error}')
    assert not misses, (kind, misses)


###############################################################################
# The multi-tensor mean
###############################################################################


@pytest.fixture(scope='module')
def chunk():
    return _lib.lib().pm_multi_mean_chunk()


def multi_mean(device, op, a, b):
    count = len(a)
    first = [t.to(device) for t in a]
    second = [first[k].detach() if t is None else t.to(device)
              for k, t in enumerate(b)]
    leaves = second if op == adversarial_oracle.ABS_DIFF else first
    for leaf in leaves:
        leaf.requires_grad_(True)
    total, means = loss._MultiMean.apply(
        (op,) * count, count, *first, *second)
    total.backward()
    out = {'means': means.detach(), 'total': total.detach().reshape(1)}
    for index, leaf in enumerate(leaves):
        assert leaf.grad.dtype == a[index].dtype
        out[f'gradient{index}'] = leaf.grad
    return out


@pytest.mark.parametrize('dtype', list(oracle.ADV_DTYPES))
@pytest.mark.parametrize('op', adversarial_oracle.OPS)
def test_multi_mean(device, chunk, op, dtype):
    kind = oracle.ADV_DTYPES[dtype]
    a, b = oracle.adversarial_inputs(op, kind, chunk)
    got_clean = multi_mean(device, op, a, b)
    for site in oracle.adversarial_plants(op, chunk):
        for name, value in oracle.VALUES.items():
            _, clean, (pa, pb), planted = oracle.adversarial_case(
                op, kind, chunk, site, value)
            compare(f'adversarial op {op} {dtype} {site} {name}', got_clean,
                    multi_mean(device, op, pa, pb), clean, planted,
                    ADVERSARIAL_GATE)


###############################################################################
# The frequency conv layer
###############################################################################

_CLEAN = {}


def frequency_layer(device, name, tensors):
    _, _, _, _, dilation, activation = fdisc_oracle.CASES[name]
    x = tensors['x'].to(device).requires_grad_(True)
    weight = tensors['weight'].to(device).requires_grad_(True)
    bias = tensors['bias'].to(device).requires_grad_(True)
    y = discriminator.frequency_conv(x, weight, bias, dilation, activation)
    y.backward(tensors['upstream'].to(device))
    return {'forward': y.detach(), 'gx': x.grad, 'gW': weight.grad,
            'gb': bias.grad}


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('site', ['x-last-pixel', 'x-inside',
                                  'upstream-inside'])
@pytest.mark.parametrize('name', oracle.FDISC_CASES)
def test_frequency_conv(device, name, site, value):
    tensors, clean, planted_tensors, planted = oracle.fdisc_case(
        name, site, oracle.VALUES[value])
    if ('fdisc', name) not in _CLEAN:
        _CLEAN['fdisc', name] = frequency_layer(device, name, tensors)
    compare(f'fdisc {name} {site} {value}', _CLEAN['fdisc', name],
            frequency_layer(device, name, planted_tensors), clean, planted,
            fdisc_oracle.gate)


###############################################################################
# The strided frequency conv layer
###############################################################################


def strided_layer(device, name, tensors):
    _, _, _, _, stride, activation = fdisc_strided_oracle.CASES[name]
    x = tensors['x'].to(device).requires_grad_(True)
    weight = tensors['weight'].to(device).requires_grad_(True)
    bias = tensors['bias'].to(device).requires_grad_(True)
    y = discriminator.frequency_conv(
        x, weight, bias, 1, activation, stride=stride)
    y.backward(tensors['upstream'].to(device))
    return {'forward': y.detach(), 'gx': x.grad, 'gW': weight.grad,
            'gb': bias.grad}


STRIDED_PLANTS = [(name, site) for name in oracle.STRIDED_CASES
                  for site in ('x-last-pixel', 'x-inside', 'upstream-inside')
                  if (name, site) != ('two-bins', 'upstream-inside')]


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('name,site', STRIDED_PLANTS)
def test_strided_frequency_conv(device, name, site, value):
    tensors, clean, planted_tensors, planted = oracle.strided_case(
        name, site, oracle.VALUES[value])
    if ('strided', name) not in _CLEAN:
        _CLEAN['strided', name] = strided_layer(device, name, tensors)
    compare(f'strided {name} {site} {value}', _CLEAN['strided', name],
            strided_layer(device, name, planted_tensors), clean, planted,
            fdisc_strided_oracle.gate)


###############################################################################
# Weight norm
###############################################################################


def weight_norm(device, tensors):
    g = tensors['g'].to(device).requires_grad_(True)
    v = tensors['v'].to(device).requires_grad_(True)
    w = discriminator.weight_norm(g, v)
    w.backward(tensors['upstream'].to(device))
    return {'forward': w.detach(), 'g_g': g.grad, 'g_v': v.grad}


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('site', list(oracle.WEIGHT_NORM_SITES))
def test_weight_norm(device, site, value):
    tensors, clean, planted_tensors, planted = oracle.weight_norm_case(
        site, oracle.VALUES[value])
    if 'weight_norm' not in _CLEAN:
        _CLEAN['weight_norm'] = weight_norm(device, tensors)
    gates = dict(zip(('forward', 'g_g', 'g_v'), fdisc_oracle.WEIGHT_NORM_GATES))
    compare(f'weight_norm {site} {value}', _CLEAN['weight_norm'],
            weight_norm(device, planted_tensors), clean, planted, gates.get)


###############################################################################
# The discriminator spectrograms
###############################################################################


def spectrogram(device, name, tensors):
    kind, sizes, _ = disc_spectrogram_oracle.CASES[name]
    leaf = tensors['x'].to(device).requires_grad_(True)
    if kind == 'R':
        out = discriminator.spectrogram_resolution(leaf, sizes)
    elif kind == 'DB':
        out = discriminator.spectrogram_decibel(leaf, sizes)
    else:
        assert (promonet_amd.WINDOW_SIZE, promonet_amd.HOPSIZE) == sizes[:2]
        out = torch.cat(discriminator.spectrogram_multiband(leaf), -1)
    out.backward(tensors['upstream'].to(device).reshape(out.shape))
    return {'forward': out.detach(), 'gx': leaf.grad}


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('site', ['x-inside', 'x-last-sample',
                                  'upstream-inside'])
@pytest.mark.parametrize('name', oracle.SPECTROGRAM_CASES)
def test_spectrogram(device, name, site, value):
    tensors, clean, planted_tensors, planted = oracle.spectrogram_case(
        name, site, oracle.VALUES[value])
    if ('spectrogram', name) not in _CLEAN:
        _CLEAN['spectrogram', name] = spectrogram(device, name, tensors)
    compare(f'spectrogram {name} {site} {value}', _CLEAN['spectrogram', name],
            spectrogram(device, name, planted_tensors), clean, planted, None,
            oracle.two_outcomes('spectrogram', name, site.split('-')[0],
                        oracle.VALUES[value]))


###############################################################################
# loss.stft, SpectralConvergence, loss.signal
###############################################################################


def loss_entry(device, entry, tensors):
    leaf = tensors['x'].to(device).requires_grad_(True)
    y = tensors['y'].to(device)
    sizes = oracle.LOSS_SIZES
    if entry == 'stft':
        window = torch.hann_window(sizes[2], dtype=torch.float64).float()
        out = loss.stft(leaf, *sizes, window.to(device))
        out.backward(tensors['upstream'].to(device))
    elif entry == 'spectral_convergence':
        out = loss.SpectralConvergence(device, *sizes)(leaf, y)
        out.backward()
    else:
        out = loss.signal(y, leaf)
        out.backward()
    out = out.detach()
    return {'forward': out if out.ndim else out.reshape(1), 'gx': leaf.grad}


LOSS_PLANTS = [(entry, site) for entry in oracle.LOSS_ENTRIES
               for site in oracle.loss_sites(entry)]


@pytest.mark.parametrize('value', VALUE_IDS)
@pytest.mark.parametrize('entry,site', LOSS_PLANTS)
def test_loss(device, entry, site, value):
    tensors, clean, planted_tensors, planted = oracle.loss_case(
        entry, site, oracle.VALUES[value])
    if ('loss', entry) not in _CLEAN:
        _CLEAN['loss', entry] = loss_entry(device, entry, tensors)
    compare(f'loss {entry} {site} {value}', _CLEAN['loss', entry],
            loss_entry(device, entry, planted_tensors), clean, planted, None,
            oracle.two_outcomes('loss', entry, site.split('-')[0],
                        oracle.VALUES[value]))


###############################################################################
# The stack and the scaler
###############################################################################


def magfree_truth(module, real, fake, hinge, step):
    """The float64 composition: the decibel spectrogram, the stack of six and
    the losses of the step (discriminator: loss.discriminator on the logits;
    generator: loss.generator on the fake logits + loss.feature_matching on
    the maps) -> (loss, whether a parameter gradient is non-finite)"""
    parameters = [
        (layer[1].weight_g.detach().cpu(), layer[1].weight_v.detach().cpu(),
         layer[1].bias.detach().cpu()) for layer in module.layers]
    dilations = [layer[1].dilation for layer in module.layers]
    logits, maps, saved = [], [], []
    for audio in (real, fake):
        x = disc_spectrogram_oracle.decibel(
            audio[:, 0], module.resolution).detach()[:, None]
        out, features, kept = fdisc_oracle.stack(x, parameters, dilations)
        logits.append(out)
        maps.append(features)
        saved.append(kept)
    if step == 'discriminator':
        total, _, _ = adversarial_oracle.discriminator(
            [logits[0]], [logits[1]], hinge)
        at_logits = adversarial_oracle.discriminator_gradient(
            [logits[0]], [logits[1]], hinge)
        upstreams = [
            [torch.zeros_like(m) for m in maps[side]] + [at_logits[side][0]]
            for side in (0, 1)]
    else:
        omit = bool(promonet_amd.config.FEATURE_MATCHING_OMIT_FIRST)
        total = adversarial_oracle.generator([logits[1]], hinge)[0] + \
            adversarial_oracle.feature_matching([maps[0]], [maps[1]], omit)
        at_maps = adversarial_oracle.feature_matching_gradient(
            [maps[0]], [maps[1]], omit)[0]
        # (the real side is a constant of the generator's step)
        upstreams = [None, at_maps + adversarial_oracle.generator_gradient(
            [logits[1]], hinge)]
    bad = False
    for kept, upstream in zip(saved, upstreams):
        if upstream is None:
            continue
        _, gradients = fdisc_oracle.stack_backward(kept, parameters, upstream)
        bad |= any(not torch.isfinite(g).all()
                   for group in gradients for g in group)
    return total, bad


@pytest.mark.parametrize('hinge', [False, True], ids=['squares', 'hinge'])
@pytest.mark.parametrize('value', [None, 'nan', 'inf'])
@pytest.mark.parametrize('step', ['discriminator', 'generator'])
def test_an_overflow_in_the_audio_reaches_the_scaler(
        device, step, value, hinge):
    """DiscriminatorMagFree([64, 16, 64]) on real and fake audio, the fake
    with one planted sample, under the losses of the discriminator's step
    (loss.discriminator) and of the generator's (loss.generator and
    loss.feature_matching, through the five maps): the loss is finite exactly
    when the truth's is,
    the statistics pass counts non-finite gradients exactly when the truth
    has one, and GradScaler.step skips the update and backs the scale off."""
    generator = torch.Generator().manual_seed(21)
    real = .1 * torch.randn(2, 1, 1024, generator=generator)
    fake = .1 * torch.randn(2, 1, 1024, generator=generator)
    if value is not None:
        fake[0, 0, 515] = oracle.VALUES[value]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(22)
        module = discriminator.DiscriminatorMagFree([64, 16, 64]).to(device)
    promonet_amd.configure(ADVERSARIAL_HINGE_LOSS=hinge)
    try:
        want_loss, want_bad = magfree_truth(
            module, real, fake, hinge, step)
        assert want_bad == (value is not None)
        parameters = [p for p in module.parameters() if p.requires_grad]
        optimizer = optim.AdamW(parameters, lr=1e-3)
        scaler = optim.GradScaler('cuda', init_scale=8.)
        real_logits, real_maps = module(real.to(device))
        fake_logits, fake_maps = module(fake.to(device))
        if step == 'discriminator':
            total, _, _ = loss.discriminator([real_logits], [fake_logits])
        else:
            total = loss.generator([fake_logits])[0] + \
                loss.feature_matching([real_maps], [fake_maps])
        scaler.scale(total).backward()
    finally:
        promonet_amd.configure(ADVERSARIAL_HINGE_LOSS=False)
    assert bool(torch.isfinite(total)) == bool(torch.isfinite(want_loss))
    stats = optim._stats_block(parameters)
    assert bool(stats[_lib.OPTIM_NONFINITE] != 0) == want_bad
    before = [p.detach().clone() for p in parameters]
    scaler.step(optimizer)
    scaler.update()
    unchanged = all(torch.equal(bits(p.detach()), bits(b))
                    for p, b in zip(parameters, before))
    assert unchanged == want_bad
    assert scaler.get_scale() == (4. if want_bad else 8.)
    if want_bad:
        for state in optimizer.state_dict()['state'].values():
            assert not state['exp_avg'].any()
            assert not state['exp_avg_sq'].any()
