"""The optimizer step of promonet_amd.optim without a GPU: the oracle
(tests/optim_oracle.py) against float64 torch.optim.AdamW, against
torch.amp.GradScaler on the CPU and against clip_grad_norm_; planted defects
that those comparisons (or the shapes of tests/test_gpu_optim.py) reject; the
state_dict round trip with torch.optim.AdamW; the ABI table and its argument
checks; and the figure behind the statistics gate of the GPU test."""
import ctypes
import math
import re
from pathlib import Path

import pytest
import torch

import promonet_amd
import promonet_amd.optim as optim
from promonet_amd import _lib

import optim_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent
EPS = 2. ** -24
ENTRIES = ('pm_optim_chunk', 'pm_optim_entries_per_launch',
           'pm_optim_workspace_bytes', 'pm_optim_grad_stats',
           'pm_optim_adamw_step', 'pm_optim_scaler_update')
HYPER = dict(lr=2e-4, betas=(.8, .99), eps=1e-9, weight_decay=1e-2)
STEPS = (1, 2, 7, 100, 5000)
SIZES = (8193, 100003)
# (gate, the largest error the oracle measures in this test) for p, m and v in
# units of 2^-24: gate = 2 x measured, over STEPS x SIZES
FLOAT64_GATES = {'p': (24.62, 12.3108), 'm': (2.128, 1.0641),
                 'v': (4.115, 2.0579)}


###############################################################################
# The oracle against float64 torch.optim.AdamW
###############################################################################


def state_inputs(numel, seed):
    """(p, g, m0, v0): gradients Gaussian times 10^U{-6..0}, the moments
    random on the gradients' scale"""
    generator = torch.Generator().manual_seed(seed)
    decade = 10. ** torch.randint(-6, 1, (numel,), generator=generator)
    def randn():
        return torch.randn(numel, generator=generator)
    return randn(), randn() * decade, randn() * decade, \
        (randn() * decade).square()


def float64_step(step, p, g, m0, v0):
    """One step of torch.optim.AdamW in float64 that arrives at `step`"""
    leaf = p.double().requires_grad_(True)
    leaf.grad = g.double()
    optimizer = torch.optim.AdamW([leaf], **HYPER)
    optimizer.state[leaf] = {
        'step': torch.tensor(float(step - 1)), 'exp_avg': m0.double().clone(),
        'exp_avg_sq': v0.double().clone()}
    optimizer.step()
    state = optimizer.state[leaf]
    return leaf.detach(), state['exp_avg'], state['exp_avg_sq']


def correct(step, p, g, m0, v0, inv_scale=1.):
    state = oracle.State(*HYPER['betas'], step=step)
    c = oracle.constants(
        state, HYPER['lr'], HYPER['eps'], HYPER['weight_decay'])
    return oracle.update(
        c, oracle.f32(inv_scale), oracle.f32(1.), g, p, m0, v0)


def errors(got, step, p, g, m0, v0):
    """The largest errors of p, m and v in units of 2^-24"""
    want = float64_step(step, p, g, m0, v0)
    lr = HYPER['lr']
    scales = (p.double().abs() + lr, m0.double().abs() + g.double().abs(),
              v0.double() + g.double().square())
    return {name: ((one.double() - other).abs() / scale).max().item() / EPS
            for name, one, other, scale in zip('pmv', got, want, scales)}


def worst(update):
    out = {'p': 0., 'm': 0., 'v': 0.}
    for step in STEPS:
        for numel in SIZES:
            inputs = state_inputs(numel, 10 * step + numel % 7)
            figures = errors(update(step, *inputs), step, *inputs)
            out = {name: max(out[name], figures[name]) for name in out}
    return out


@pytest.fixture(scope='module')
def measured():
    return worst(correct)


def test_the_oracle_follows_float64_adamw(measured):
    print('oracle against float64 torch.optim.AdamW, x 2^-24:',
          {name: round(value, 4) for name, value in measured.items()})
    for name, (gate, recorded) in FLOAT64_GATES.items():
        assert measured[name] < gate, (name, measured[name])
        # the gates are 2 x what this test measures
        assert recorded < gate <= 2.001 * recorded
        assert abs(measured[name] - recorded) <= 1e-3 * recorded, \
            (name, measured[name], recorded)


def test_the_oracles_root_and_quotient_are_correctly_rounded():
    """Against their definitions, in float64 products that are exact: s is
    the fp32 nearest to sqrt(v) if v lies between the squares of s -+ half an
    ulp (25 bits each, 50 bits squared), and q the one nearest to a / b if
    |a - q b| <= half an ulp of q times |b| (q b has 48 bits; the difference
    of two doubles that close is exact)"""
    v = oracle.decades((100003,), 11).square() + 1e-30
    a = oracle.decades((100003,), 12)
    b = oracle.decades((100003,), 13).abs() + 1e-12
    s = oracle.sqrt(v).double()
    half = (torch.nextafter(s.float(), torch.tensor(math.inf)).double() - s) / 2
    lower = s - torch.where(s == 2. ** torch.floor(torch.log2(s)),
                            half / 2, half)
    assert ((lower * lower <= v.double()) &
            (v.double() <= (s + half) * (s + half))).all()
    q = (a / b).double()
    half = (torch.nextafter(q.float().abs(), torch.tensor(math.inf)).double()
            - q.abs()) / 2
    assert ((a.double() - q * b.double()).abs() <= half * b.double()).all()


###############################################################################
# Planted defects
###############################################################################


def defective(kind):
    """The update with one planted defect"""
    def update(step, p, g, m0, v0):
        lr, eps, wd = HYPER['lr'], HYPER['eps'], HYPER['weight_decay']
        state = oracle.State(
            *HYPER['betas'], step=step - 1 if kind == 'step - 1' else step)
        if kind == 'step - 1' and step == 1:
            # (1 - beta^0 is 0: the defect divides by zero at the first step)
            state.b1pow = state.b2pow = 1. - 2. ** -53
        c = oracle.constants(state, lr, eps, wd)
        m = m0 + c['one_minus_beta1'] * (g - m0)
        v = v0 * c['beta2'] + c['one_minus_beta2'] * (g * g)
        if kind == 'eps inside the root':
            d = oracle.sqrt(v + c['eps']) / c['bias2']
        else:
            d = oracle.sqrt(v) / c['bias2'] + c['eps']
        if kind == 'decay after the update':
            p = p + c['step'] * (m / d)
            p = p * c['decay']
        else:
            p = p * c['decay']
            p = p + c['step'] * (m / d)
        return p, m, v
    return update


def test_the_defect_free_restatement_is_the_oracle():
    inputs = state_inputs(8193, 3)
    for one, other in zip(defective(None)(7, *inputs), correct(7, *inputs)):
        assert torch.equal(one, other)


@pytest.mark.parametrize(
    'kind', ('step - 1', 'decay after the update', 'eps inside the root'))
def test_float64_adamw_rejects_a_planted_defect(kind):
    figures = worst(defective(kind))
    print(kind, {name: round(value, 2) for name, value in figures.items()})
    assert figures['p'] >= FLOAT64_GATES['p'][0], figures


def test_a_skipped_unscale_is_rejected():
    """Gradients scaled by 2^16 against float64 AdamW on the unscaled ones:
    with the unscale the gates hold, without it they do not"""
    p, g, m0, v0 = state_inputs(8193, 5)
    scaled = g * 2. ** 16
    def figures(inv_scale):
        got = correct(7, p, scaled, m0, v0, inv_scale)
        return errors(got, 7, p, g, m0, v0)
    good, bad = figures(2. ** -16), figures(1.)
    assert all(good[n] < FLOAT64_GATES[n][0] for n in 'pmv'), good
    assert all(bad[n] >= FLOAT64_GATES[n][0] for n in 'mv'), bad


def test_moments_written_on_a_skipped_step_are_rejected():
    """The oracle leaves p, m, v and the state alone when found_inf is set;
    an update that wrote the moments would differ in every one"""
    params = [oracle.gaussian((100,), 1), oracle.gaussian((7,), 2)]
    ref = oracle.AdamW(params, 2048)
    good = [oracle.gaussian((100,), 3, 1e-2), oracle.gaussian((7,), 4, 1e-2)]
    assert not ref.step(good)
    before = [t.clone() for t in ref.params + ref.exp_avg + ref.exp_avg_sq]
    for planted, incoming in ((math.inf, 0.), (math.nan, 0.), (None, 1.)):
        grads = [g.clone() for g in good]
        if planted is not None:
            grads[1][-1] = planted
        assert ref.step(grads, found_inf=incoming)
        assert ref.last['nonfinite'] == (planted is not None)
        assert (ref.state.step, ref.state.b1pow, ref.state.b2pow) == \
            (1, .8, .99)
        after = ref.params + ref.exp_avg + ref.exp_avg_sq
        assert all(torch.equal(a, b) for a, b in zip(after, before))
        # the planted defect: the moments of the finite entries move
        c = oracle.constants(ref.state, ref.lr, ref.eps, ref.weight_decay)
        _, m, v = oracle.update(c, oracle.f32(1.), oracle.f32(1.), grads[0],
                                ref.params[0], ref.exp_avg[0],
                                ref.exp_avg_sq[0])
        assert not torch.equal(m, before[2]) and not torch.equal(v, before[4])


def test_the_table_of_the_gpu_test_rejects_an_off_by_one_chunk_boundary():
    """A pass that loses the element on either side of a chunk boundary (the
    last one of a whole chunk, or the first one after it) gives another sum
    of squares on the Gaussian gradients of the GPU test: its sizes of one
    chunk, one more and several chunks with a tail tell both"""
    import test_gpu_optim as gpu
    chunk = _lib.lib().pm_optim_chunk()
    per_launch = _lib.lib().pm_optim_entries_per_launch()
    table = gpu.sizes(chunk, per_launch)
    assert {(chunk - 1, 0), (chunk, 0), (chunk + 1, 0),
            (3 * chunk + 5, 0)} <= set(table)
    grads = gpu.gaussian_gradients(chunk, per_launch, torch.float32)
    right = oracle.grad_stats(grads, chunk)['norm_sq']
    for lost in (chunk - 1, chunk):
        kept = []
        for g in grads:
            keep = torch.ones(g.numel(), dtype=torch.bool)
            keep[lost::chunk] = False
            kept.append(torch.where(keep, g, torch.zeros_like(g)))
        assert sum(int((k != g).sum()) for k, g in zip(kept, grads)) >= 4
        wrong = oracle.grad_stats(kept, chunk)['norm_sq']
        assert not torch.equal(wrong, right), lost
    # A pass that loses nothing but cuts its chunks one element early only
    # changes the order of the sums, which shows where it moves a rounded
    # figure. The GPU test holds every statistic to the restatement bit for
    # bit, and on its fp32 gradients that cut gives another mean: caught.
    # (In the update a wrong boundary leaves an element of p, m and v
    # unwritten or writes past the chunk: the bit-for-bit table sees both.)
    right = oracle.grad_stats(grads, chunk)['mean']
    total = sum(g.numel() for g in grads)
    cut = chunk - 1
    partials = torch.cat([
        oracle.chunk_partials(g[start:start + cut], chunk)
        for g in grads for start in range(0, g.numel(), cut)])
    wrong = oracle.f32(oracle.ordered_sum(partials) / total)
    assert not torch.equal(wrong, right)


###############################################################################
# The scaler and the clip against torch
###############################################################################


def test_the_scaler_rule_equals_torch_on_the_cpu():
    """init_scale 4, growth_interval 2, the steps finite, finite, inf,
    finite, finite: the scale, the tracker and the skipped step"""
    leaf = torch.ones(3, requires_grad=True)
    optimizer = torch.optim.SGD([leaf], lr=1.)
    scaler = torch.amp.GradScaler('cpu', init_scale=4., growth_interval=2)
    ref = oracle.AdamW([torch.ones(3)], 2048)
    scale, tracker, scales = 4., 0, []
    for overflow in (0, 0, 1, 0, 0):
        optimizer.zero_grad()
        weight = torch.tensor([1., math.inf if overflow else 2., 3.])
        scaler.scale((leaf * weight).sum()).backward()
        grads = [leaf.grad.clone()]
        before = leaf.detach().clone()
        scaler.step(optimizer)
        scaler.update()
        skipped = torch.equal(leaf.detach(), before)
        found = ref.step(grads, scale)
        assert found == skipped == bool(overflow)
        scale, tracker = oracle.scaler_update(
            scale, tracker, found, interval=2)
        assert scaler.get_scale() == scale
        assert scaler._get_growth_tracker() == tracker
        scales.append(scale)
    assert scales == [4., 8., 4., 4., 8.]
    assert ref.state.step == 4
    # growth that would be inf is not taken; other factors round as torch's
    assert oracle.scaler_update(3e38, 0, False, interval=1) == (3e38, 0)
    for factor in (1.1, 1.7):
        cell = torch.tensor(float(oracle.f32(3.3)))
        torch._amp_update_scale_(
            cell, torch.zeros(1, dtype=torch.int32), torch.zeros(1), factor,
            .5, 1)
        assert oracle.scaler_update(
            float(oracle.f32(3.3)), 0, False, factor, .5, 1)[0] == cell.item()


@pytest.mark.parametrize('clip,scale,binds', (
    (1e-2, 1., True), (10., 1., False), (1e-2, 2. ** 16, True),
    (1e3, 2. ** 16, False), (1e6, 2. ** 16, False)))
def test_the_clip_rule_equals_clip_grad_norm(clip, scale, binds):
    """The reference's order (train/core.py:347-363): the scaled maximum
    against the threshold, then unscale and clip_grad_norm_(norm_type='inf');
    the gradient the update then uses is the oracle's (g inv_scale) coef to
    the bit. With clip = 1e3 the scaled maximum is above the threshold and
    the unscaled one below: torch clamps the coefficient to 1."""
    grads = [oracle.gaussian((1000,), 1, 1e-1) * scale,
             oracle.gaussian((37,), 2, 1e-1) * scale]
    stats = oracle.grad_stats(grads, 2048)
    found, inv_scale, coef = oracle.control(stats, scale, 0., clip)
    assert not found and (coef < 1) == binds
    ours = [(g * inv_scale) * coef for g in grads]
    # torch
    leaves = [torch.zeros_like(g).requires_grad_(True) for g in grads]
    for leaf, g in zip(leaves, grads):
        leaf.grad = g.clone()
    largest = max(max(g.max().item() for g in grads),
                  abs(min(g.min().item() for g in grads)))
    unscale = torch.tensor(scale).double().reciprocal().float()
    if largest > clip:
        for leaf in leaves:
            leaf.grad.mul_(unscale)
        torch.nn.utils.clip_grad_norm_(leaves, clip, norm_type='inf')
    else:
        # scaler.step() unscales what was left alone
        assert coef == 1
        for leaf in leaves:
            leaf.grad.mul_(unscale)
    for leaf, want in zip(leaves, ours):
        assert torch.equal(leaf.grad, want)


###############################################################################
# state_dict
###############################################################################


def test_state_dict_round_trips_with_torch_on_the_cpu():
    generator = torch.Generator().manual_seed(0)
    shapes = ((3, 4), (5,), (2, 3, 2))

    def leaves():
        return [torch.randn(s, generator=generator).requires_grad_(True)
                for s in shapes]

    theirs = torch.optim.AdamW(leaves(), **HYPER)
    for _ in range(3):
        for leaf in theirs.param_groups[0]['params']:
            leaf.grad = torch.randn(leaf.shape, generator=generator)
        theirs.step()
    saved = theirs.state_dict()
    # torch's -> ours -> torch's: the same state
    ours = optim.AdamW(leaves())
    ours.load_state_dict(saved)
    back = ours.state_dict()
    assert back['state'].keys() == saved['state'].keys()
    for index, state in saved['state'].items():
        assert set(back['state'][index]) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert float(back['state'][index]['step']) == 3
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(back['state'][index][key], state[key])
    assert back['param_groups'][0]['params'] == \
        saved['param_groups'][0]['params']
    again = torch.optim.AdamW(leaves(), **HYPER)
    again.load_state_dict(back)
    for leaf, other in zip(again.param_groups[0]['params'],
                           theirs.param_groups[0]['params']):
        assert torch.equal(again.state[leaf]['exp_avg'],
                           theirs.state[other]['exp_avg'])
        assert again.state[leaf]['step'] == 3
    # one step for the optimizer: parameters at different steps do not load
    saved['state'][1]['step'] = torch.tensor(5.)
    with pytest.raises(ValueError, match='different steps'):
        optim.AdamW(leaves()).load_state_dict(saved)


###############################################################################
# The ABI and the Python entry points
###############################################################################


def test_the_constants_agree():
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    for name in ('MAX', 'MIN', 'MEAN', 'NORM', 'NORM_SQ', 'NONFINITE',
                 'FOUND_INF', 'INV_SCALE', 'COEF', 'STATS'):
        value = int(re.search(
            rf'#define PM_OPTIM_{name} (\d+)', header).group(1))
        assert value == getattr(_lib, f'OPTIM_{name}')
    assert optim.STATS_KEYS == (
        'gradients/max', 'gradients/min', 'gradients/mean', 'gradients/norm')
    # nothing imports the module unless asked
    source = (ROOT / 'promonet_amd' / '__init__.py').read_text()
    assert 'optim' not in source


def test_abi_entries_and_their_argument_checks():
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    declared = set(re.findall(r'\b(pm_[a-z0-9_]+)\s*\(', header))
    library = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in declared, name
        assert hasattr(library, name), name
    chunk = library.pm_optim_chunk()
    per_launch = library.pm_optim_entries_per_launch()
    assert chunk > 0 and chunk % (oracle.THREADS * oracle.VEC) == 0
    # an entry is four pointers, a count and a word: the table of a launch and
    # the other arguments stay under 4 KB
    assert 0 < per_launch * 48 + 16 + 128 <= 4096

    def longs(*values):
        return (ctypes.c_longlong * len(values))(*values)

    def ints(*values):
        return (ctypes.c_int * len(values))(*values)

    def pointers(*values):
        return (ctypes.c_void_p * len(values))(*values)

    # the workspace: five values a chunk, each array rounded to 256 bytes
    size = library.pm_optim_workspace_bytes
    assert size(longs(1, chunk, chunk + 1), 3) == 5 * 256
    assert size(longs(65 * chunk), 1) == 5 * 512
    assert size(None, 1) == 0
    assert size(longs(5), 0) == 0
    assert size(longs(5, 0), 2) == 0
    assert size(longs(-1), 1) == 0

    # every bad argument answers -1 before any device work (the pointers are
    # made up and never followed)
    fake = 0x1000
    good = dict(p=pointers(fake), m=pointers(fake), v=pointers(fake),
                g=pointers(fake), numel=longs(5), dtype=ints(0), count=1,
                stats=fake, state=fake, workspace=fake, size=1 << 20,
                clip=-1., lr=2e-4, beta1=.8, beta2=.99, eps=1e-9, wd=1e-2)

    def stats(**changes):
        v = dict(good, **changes)
        return library.pm_optim_grad_stats(
            v['g'], v['numel'], v['dtype'], v['count'], None, None, v['clip'],
            v['beta1'], v['beta2'], v['state'], v['stats'], v['workspace'],
            v['size'], None)

    def step(**changes):
        v = dict(good, **changes)
        return library.pm_optim_adamw_step(
            v['p'], v['m'], v['v'], v['g'], v['numel'], v['dtype'],
            v['count'], v['stats'], v['state'], v['lr'], v['beta1'],
            v['beta2'], v['eps'], v['wd'], None)

    for changes in (dict(count=0), dict(count=-3), dict(g=None),
                    dict(numel=None), dict(dtype=None), dict(numel=longs(0)),
                    dict(numel=longs(-7)), dict(dtype=ints(3)),
                    dict(dtype=ints(-1)), dict(g=pointers(None)),
                    dict(stats=None), dict(beta1=1.), dict(beta2=-.1)):
        assert stats(**changes) == -1, changes
        assert library.pm_last_error()
        assert step(**changes) == -1, changes
    assert stats(workspace=None) == -1
    assert stats(clip=math.nan) == -1
    assert stats(size=5 * 256 - 1) == -1
    assert b'workspace' in library.pm_last_error()
    for changes in (dict(p=None), dict(m=None), dict(v=None),
                    dict(p=pointers(None)), dict(m=pointers(None)),
                    dict(v=pointers(None)), dict(state=None), dict(lr=-1.),
                    dict(eps=-1.), dict(wd=-1.), dict(lr=math.nan)):
        assert step(**changes) == -1, changes

    def scaler(**changes):
        v = dict(dict(scale=fake, tracker=fake, found=pointers(fake), count=1,
                      growth=2., backoff=.5, interval=2000), **changes)
        return library.pm_optim_scaler_update(
            v['scale'], v['tracker'], v['found'], v['count'], v['growth'],
            v['backoff'], v['interval'], None)

    for changes in (dict(scale=None), dict(tracker=None), dict(found=None),
                    dict(found=pointers(None)), dict(count=0), dict(count=9),
                    dict(growth=1.), dict(backoff=1.), dict(backoff=0.),
                    dict(interval=0)):
        assert scaler(**changes) == -1, changes


def test_value_errors_come_before_any_device_work():
    with pytest.raises(ValueError, match='fp32'):
        optim.AdamW([torch.zeros(3, dtype=torch.float16)])
    with pytest.raises(ValueError, match='fp32'):
        optim.AdamW([torch.zeros(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match='contiguous'):
        optim.AdamW([torch.zeros(3, 4).t()])
    with pytest.raises(ValueError, match='betas'):
        optim.AdamW([torch.zeros(3)], betas=(1., .99))
    with pytest.raises(ValueError, match='clip'):
        optim.AdamW([torch.zeros(3)], clip=-1.)
    with pytest.raises(ValueError, match='same betas'):
        optim.AdamW([{'params': [torch.zeros(3)]},
                     {'params': [torch.zeros(2)], 'betas': (.9, .99)}])
    with pytest.raises(ValueError, match='no parameter has a gradient'):
        optim.gradient_stats([torch.zeros(3)])
    # a step with no gradient does nothing; there is no CPU fallback
    leaf = torch.zeros(3, requires_grad=True)
    optimizer = optim.AdamW([leaf])
    assert optimizer.defaults == dict(
        lr=2e-4, betas=(.8, .99), eps=1e-9, weight_decay=1e-2)
    optimizer.step()
    leaf.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        optimizer.step()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        optim.gradient_stats([leaf])
    assert optimizer._step_supports_amp_scaling is True
    # a scaler that is not on a GPU, or another optimizer, is torch's
    assert issubclass(optim.GradScaler, torch.amp.GradScaler)
    assert optim.GradScaler('cpu').state_dict().keys() == \
        torch.amp.GradScaler('cpu').state_dict().keys()


###############################################################################
# The conditions of tests/test_gpu_optim.py
###############################################################################


def test_the_statistics_gate_is_three_times_the_restatement():
    import test_gpu_optim as gpu
    chunk = _lib.lib().pm_optim_chunk()
    per_launch = _lib.lib().pm_optim_entries_per_launch()
    worst = max(gpu.restatement_figure(chunk, per_launch, dtype)
                for dtype in gpu.DTYPES)
    gate, recorded = gpu.STATS_GATE
    print(f'gate {gate}, recorded {recorded}, fp32 CPU {worst:.4f}')
    assert abs(worst - recorded) <= 1e-3 * recorded
    assert recorded < gate <= 3.001 * recorded


def test_the_grid_keeps_every_sum_exact():
    import test_gpu_optim as gpu
    chunk = _lib.lib().pm_optim_chunk()
    per_launch = _lib.lib().pm_optim_entries_per_launch()
    for dtype in gpu.DTYPES:
        grads = gpu.grid_gradients(chunk, per_launch, dtype)
        gpu.assert_sums_are_exact(grads, chunk)
        # so the restatement is the float64 value rounded once
        got = oracle.grad_stats(grads, chunk)
        every = torch.cat([g.double() for g in grads])
        assert torch.equal(got['mean'], (every.sum() / every.numel()).float())
        assert torch.equal(got['norm_sq'], every.square().sum().float())
        assert got['max'] == every.max() and got['min'] == every.min()
