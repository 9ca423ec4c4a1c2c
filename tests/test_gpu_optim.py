"""The optimizer step on the GPU (pm_optim.h through promonet_amd.optim)
against tests/optim_oracle.py.

The update is held to the oracle bit for bit (`torch.equal`): p, m and v after
each of three consecutive steps, for gradients stored as fp32, f16 and bf16,
with and without a loss scale of 2^16, and the control block with them. The
inputs stay in the normal range of fp32 (and of f16 where they are stored as
f16): what the device does with denormals is NOT pinned by these tests.

The statistics: on a dyadic grid every sum is exact (asserted from the
inputs), so max, min, mean and norm^2 equal the float64 values rounded once;
on Gaussian inputs the device equals the oracle's chunked restatement bit for
bit, and against float64 the gate is 3 x the figure that restatement itself
reaches on the same inputs (STATS_GATE; tests/test_cpu_optim.py asserts it).
"""
import ctypes
import functools

import pytest
import torch

import promonet_amd
import promonet_amd.optim as optim
from promonet_amd import _lib

import adversarial_oracle
import optim_oracle as oracle
from util import check

EPS = 2. ** -24
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
DTYPE_IDS = ('fp32', 'f16', 'bf16')
SCALE = 2. ** 16
# (the gate, the figure of the fp32 CPU restatement in the kernel's order on
# gaussian_gradients(), largest over the three dtypes, in units of 2^-24):
# gate = 3 x the figure. The device's figures are the restatement's, because
# its sums are the restatement's bit for bit (asserted below).
STATS_GATE = (4.42, 1.4742)


def sizes(chunk, per_launch):
    """(numel, storage offset): one element, less than a wave, around one
    chunk, several chunks with a tail, a view that is not 16-byte aligned,
    and 2 launches + 3 tensors of 17 elements"""
    return ((1, 0), (63, 0), (chunk - 1, 0), (chunk, 0), (chunk + 1, 0),
            (3 * chunk + 5, 0), (chunk + 3, 1)) + \
        ((17, 0),) * (2 * per_launch + 3)


###############################################################################
# Inputs (CPU tensors; computed once and left unchanged)
###############################################################################


@functools.lru_cache(maxsize=None)
def parameters(chunk, per_launch):
    return tuple(oracle.gaussian((numel,), 1000 + k)
                 for k, (numel, _) in enumerate(sizes(chunk, per_launch)))


@functools.lru_cache(maxsize=None)
def gradients(chunk, per_launch, step, dtype, scaled=False):
    """Magnitudes from 0.25 to about 5 times 10^-2 or 10^-3, away from zero
    (normal in f16, and their squares times 1 - beta2 normal in fp32), stored
    in `dtype`, times 2^16 when scaled (at most about 3 400: finite in f16)"""
    out = []
    for k, (numel, _) in enumerate(sizes(chunk, per_launch)):
        value = oracle.gaussian((numel,), 2000 + 1000 * step + k)
        value = (value.abs() + .25) * torch.where(value < 0, -1., 1.) * \
            10. ** (-2 - k % 2)
        out.append((value * (SCALE if scaled else 1.)).to(dtype))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def grid_gradients(chunk, per_launch, dtype):
    return tuple(
        adversarial_oracle.grid((numel,), 2. ** -4, 3000 + k, dtype)
        for k, (numel, _) in enumerate(sizes(chunk, per_launch)))


@functools.lru_cache(maxsize=None)
def gaussian_gradients(chunk, per_launch, dtype):
    return tuple(oracle.gaussian((numel,), 4000 + k).to(dtype)
                 for k, (numel, _) in enumerate(sizes(chunk, per_launch)))


def assert_sums_are_exact(grads, chunk):
    """From the inputs: every gradient is a multiple of 2^-4 and every square
    one of 2^-8, and inside a chunk both sums over their unit stay below
    2^24, so every fp32 partial sum is exact whatever the order; the chunks
    are added in double, which holds the sums of the whole list exactly"""
    total = 0.
    for g in grads:
        g = g.double()
        assert torch.equal(g * 16, (g * 16).round())
        for start in range(0, g.numel(), chunk):
            part = g[start:start + chunk]
            assert (part.abs() * 16).sum().item() < 2. ** 24
            assert (part.square() * 256).sum().item() < 2. ** 24
        total += (g.square() * 256).sum().item()
    assert total < 2. ** 53


def stats_figure(got, grads):
    """The largest error of mean (relative to the mean magnitude), norm and
    norm^2 against float64, in units of 2^-24"""
    mean, norm, norm_sq, magnitude = oracle.grad_stats_float64(grads)
    return max(
        ((got['mean'].double() - mean).abs() / magnitude).item(),
        ((got['norm'].double() - norm).abs() / norm).item(),
        ((got['norm_sq'].double() - norm_sq).abs() / norm_sq).item()) / EPS


@functools.lru_cache(maxsize=None)
def restatement(chunk, per_launch, dtype):
    return oracle.grad_stats(
        gaussian_gradients(chunk, per_launch, dtype), chunk)


def restatement_figure(chunk, per_launch, dtype):
    return stats_figure(restatement(chunk, per_launch, dtype),
                        gaussian_gradients(chunk, per_launch, dtype))


###############################################################################
# Through the kernels
###############################################################################


def on_device(tensor, device, offset=0):
    """A copy on the device that starts `offset` elements into its storage"""
    storage = torch.empty(
        tensor.numel() + offset, dtype=tensor.dtype, device=device)
    view = storage[offset:].view(tensor.shape)
    view.copy_(tensor)
    assert view.storage_offset() == offset
    return view


def leaves(device, table, values, dtype=torch.float32):
    """The parameters on the device; their gradients are kept in `dtype`"""
    out = []
    for (_, offset), value in zip(table, values):
        leaf = on_device(value, device, offset).requires_grad_(True)
        if dtype != torch.float32:
            leaf.grad_dtype = dtype
        out.append(leaf)
    return out


def give(leaves, table, grads, device):
    for leaf, (_, offset), g in zip(leaves, table, grads):
        leaf.grad = None if g is None else on_device(g, device, offset)


def block(stats):
    """The named floats of a statistics block, on the CPU"""
    stats = stats.cpu()
    return {name: stats[getattr(_lib, f'OPTIM_{name.upper()}')]
            for name in ('max', 'min', 'mean', 'norm', 'norm_sq', 'nonfinite',
                         'found_inf', 'inv_scale', 'coef')}


def assert_block(optimizer, ref):
    got = block(optimizer._stats)
    for name, want in ref.last.items():
        assert torch.equal(got[name], want), (name, got[name], want)
    state = optimizer._state.cpu().tolist()
    assert state == [float(ref.state.step), ref.state.b1pow, ref.state.b2pow]


def assert_tensors(optimizer, params, ref, where):
    for k, p in enumerate(params):
        state = optimizer.state[p]
        assert torch.equal(p.detach().cpu(), ref.params[k]), (where, k, 'p')
        assert torch.equal(state['exp_avg'].cpu(), ref.exp_avg[k]), \
            (where, k, 'm')
        assert torch.equal(state['exp_avg_sq'].cpu(), ref.exp_avg_sq[k]), \
            (where, k, 'v')


@pytest.fixture(scope='module')
def chunk():
    return _lib.lib().pm_optim_chunk()


@pytest.fixture(scope='module')
def per_launch():
    return _lib.lib().pm_optim_entries_per_launch()


@pytest.mark.gpu
@pytest.mark.parametrize('scaled', (False, True), ids=('unscaled', 'scaled'))
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_three_steps_equal_the_oracle(device, chunk, per_launch, dtype,
                                      scaled):
    table = sizes(chunk, per_launch)
    assert len(table) == 7 + 2 * per_launch + 3
    values = parameters(chunk, per_launch)
    params = leaves(device, table, values, dtype)
    optimizer = optim.AdamW(params)
    ref = oracle.AdamW(values, chunk)
    scale = torch.tensor(SCALE, device=device)
    for step in range(3):
        grads = gradients(chunk, per_launch, step, dtype, scaled)
        assert all(g.float().abs().min() >= 6.2e-5 and
                   torch.isfinite(g).all() for g in grads)
        give(params, table, grads, device)
        assert all(p.grad.dtype == dtype for p in params)
        if scaled:
            # torch's protocol for fused optimizers
            optimizer.grad_scale = scale
            optimizer.found_inf = torch.zeros((), device=device)
        optimizer.step()
        assert not ref.step(grads, SCALE if scaled else None)
        assert_block(optimizer, ref)
        assert_tensors(optimizer, params, ref, step)
        assert all(torch.isfinite(p).all() and p.abs().min() > 1e-30
                   for p in ref.exp_avg_sq)
    assert ref.state.step == 3


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_statistics_are_exact_on_the_grid(device, chunk, per_launch, dtype):
    table = sizes(chunk, per_launch)
    grads = grid_gradients(chunk, per_launch, dtype)
    assert_sums_are_exact(grads, chunk)
    params = leaves(device, table, parameters(chunk, per_launch), dtype)
    give(params, table, grads, device)
    got = block(optim._stats_block(params))
    every = torch.cat([g.double() for g in grads])
    assert torch.equal(got['max'], every.max().float())
    assert torch.equal(got['min'], every.min().float())
    assert torch.equal(got['mean'], (every.sum() / every.numel()).float())
    assert torch.equal(got['norm_sq'], every.square().sum().float())
    assert torch.equal(got['norm'], every.square().sum().sqrt().float())
    assert got['nonfinite'] == 0 and got['found_inf'] == 0
    assert got['inv_scale'] == 1 and got['coef'] == 1
    # the public entry: the same four figures, nothing else
    public = optim.gradient_stats(params)
    assert set(public) == set(optim.STATS_KEYS)
    for key, value in public.items():
        assert value.ndim == 0 and value.device.type == 'cuda'
        assert torch.equal(value.cpu(), got[key.split('/')[1]])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_statistics_of_gaussian_gradients(device, chunk, per_launch, dtype):
    table = sizes(chunk, per_launch)
    grads = gaussian_gradients(chunk, per_launch, dtype)
    params = leaves(device, table, parameters(chunk, per_launch), dtype)
    give(params, table, grads, device)
    got = block(optim._stats_block(params))
    want = restatement(chunk, per_launch, dtype)
    measured = stats_figure(got, grads)
    print(f'gaussian statistics {dtype}: {measured:.4f} x 2^-24 (fp32 CPU '
          f'restatement {restatement_figure(chunk, per_launch, dtype):.4f})')
    check(measured, STATS_GATE[0], 'optim/gaussian_statistics', dtype)
    for name, value in want.items():
        assert torch.equal(got[name], value), (name, got[name], value)


def planted(chunk, per_launch, value):
    """Finite gradients with `value` in the last element of the last tensor
    of the second launch"""
    grads = list(gradients(chunk, per_launch, 0, torch.float32))
    last = 2 * per_launch - 1
    grads[last] = grads[last].clone()
    grads[last][-1] = value
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize('case', ('inf', 'nan', 'incoming'))
def test_a_step_with_a_non_finite_gradient_is_skipped(
        device, chunk, per_launch, case):
    table = sizes(chunk, per_launch)
    values = parameters(chunk, per_launch)
    params = leaves(device, table, values)
    optimizer = optim.AdamW(params)
    ref = oracle.AdamW(values, chunk)
    scaler = optim.GradScaler('cuda', init_scale=4., growth_interval=2)
    scaler.scale(torch.zeros(1, device=device))
    # one good step, so that the moments and the step are not zero
    good = gradients(chunk, per_launch, 1, torch.float32)
    give(params, table, good, device)
    scaler.step(optimizer)
    scaler.update()
    assert not ref.step(good, 4.)
    assert_tensors(optimizer, params, ref, 'before')
    before = [(p.detach().clone(), optimizer.state[p]['exp_avg'].clone(),
               optimizer.state[p]['exp_avg_sq'].clone()) for p in params]
    if case == 'incoming':
        grads = list(gradients(chunk, per_launch, 0, torch.float32))
        give(params, table, grads, device)
        optimizer.grad_scale = torch.tensor(4., device=device)
        optimizer.found_inf = torch.ones((), device=device)
        optimizer.step()
        del optimizer.grad_scale, optimizer.found_inf
        assert ref.step(grads, 4., found_inf=1.)
        got = block(optimizer._stats)
        assert got['nonfinite'] == 0 and got['found_inf'] == 1
        # the scalar reaches the scaler beside a second optimizer's, which
        # found nothing: two scalars in one update
        other = torch.zeros(1, device=device)
        states = scaler._per_optimizer_states
        states[id(optimizer)]['found_inf_per_device'] = {
            device: optimizer.found_inf_scalar()}
        states['other']['found_inf_per_device'] = {device: other}
        scaler.update()
        assert scaler.get_scale() == 2. and scaler._get_growth_tracker() == 0
        assert optimizer.found_inf_scalar().item() == 0 and other.item() == 0
    else:
        grads = planted(chunk, per_launch,
                        float('inf') if case == 'inf' else float('nan'))
        give(params, table, grads, device)
        scaler.step(optimizer)
        assert ref.step(grads, 4.)
        got = block(optimizer._stats)
        assert got['nonfinite'] == 1 and got['found_inf'] == 1
        scaler.update()
        # the scaler backs off, and clears what it read
        assert scaler.get_scale() == 2. and scaler._get_growth_tracker() == 0
        assert optimizer.found_inf_scalar().item() == 0
        assert oracle.scaler_update(4., 1, True, interval=2) == (2., 0)
    assert ref.last['found_inf'] == 1
    # the step, the powers, p, m and v are unchanged bit for bit
    state = optimizer._state.cpu().tolist()
    assert state == [1., ref.state.b1pow, ref.state.b2pow] == [1., .8, .99]
    for p, (old_p, old_m, old_v) in zip(params, before):
        assert torch.equal(p.detach(), old_p)
        assert torch.equal(optimizer.state[p]['exp_avg'], old_m)
        assert torch.equal(optimizer.state[p]['exp_avg_sq'], old_v)
    assert_tensors(optimizer, params, ref, 'after')
    figures = optimizer.stats()
    assert set(figures) == set(optim.STATS_KEYS) | {'gradients/nonfinite'}
    assert all(f.device.type == 'cuda' for f in figures.values())


@pytest.mark.gpu
@pytest.mark.parametrize('clip,scaled,binds', (
    (1e-3, False, True), (1e3, False, False), (1e-3, True, True),
    (1e3, True, False)))
def test_the_clip_equals_the_oracle(device, chunk, per_launch, clip, scaled,
                                    binds):
    """(with the scale 2^16 and clip = 1e3 the scaled maximum is above the
    threshold and the unscaled one is not: the coefficient clamps to 1)"""
    table = sizes(chunk, per_launch)[:12]
    values = parameters(chunk, per_launch)[:12]
    params = leaves(device, table, values)
    optimizer = optim.AdamW(params, clip=clip)
    ref = oracle.AdamW(values, chunk, clip=clip)
    for step in range(2):
        grads = gradients(chunk, per_launch, step, torch.float32, scaled)[:12]
        give(params, table, grads, device)
        if scaled:
            optimizer.grad_scale = torch.tensor(SCALE, device=device)
        optimizer.step()
        ref.step(grads, SCALE if scaled else None)
        assert (ref.last['coef'] < 1) == binds
        assert_block(optimizer, ref)
        assert_tensors(optimizer, params, ref, step)


@pytest.mark.gpu
def test_a_step_after_unscale_takes_the_gradients_as_they_are(
        device, chunk, per_launch):
    """The reference's loop where the clip binds: scaler.unscale_(optimizer)
    runs torch's pass, then scaler.step(optimizer) hands over no scale and
    torch's found_inf. A finite step, then one with an inf."""
    table = sizes(chunk, per_launch)[:9]
    values = parameters(chunk, per_launch)[:9]
    params = leaves(device, table, values)
    optimizer = optim.AdamW(params, clip=1e-3)
    ref = oracle.AdamW(values, chunk, clip=1e-3)
    scaler = optim.GradScaler('cuda', init_scale=4., growth_interval=2)
    scaler.scale(torch.zeros(1, device=device))
    for step, overflow in enumerate((False, True)):
        unscaled = [g.clone() for g in
                    gradients(chunk, per_launch, step, torch.float32)[:9]]
        if overflow:
            unscaled[5][-1] = float('inf')
        give(params, table, [g * 4. for g in unscaled], device)
        scaler.unscale_(optimizer)
        assert all(torch.equal(p.grad.cpu(), g)
                   for p, g in zip(params, unscaled))
        scaler.step(optimizer)
        # (torch's pass found the inf; the statistics pass counts it too)
        assert ref.step(unscaled, None, found_inf=float(overflow)) == overflow
        assert ref.last['coef'] < 1
        assert_block(optimizer, ref)
        assert_tensors(optimizer, params, ref, step)
        scaler.update()
        assert scaler.get_scale() == (2. if overflow else 4.)
    assert optimizer._state[0].item() == 1


@pytest.mark.gpu
def test_one_scaler_over_ten_optimizers(device, chunk):
    """More found_inf scalars than one scaler kernel reads: they are added
    first. One optimizer of ten meets a NaN: it alone is skipped, and the
    scale backs off; a round without one counts towards the growth."""
    values = [oracle.gaussian((33,), 600 + k) for k in range(10)]
    params = leaves(device, [(33, 0)] * 10, values)
    optimizers = [optim.AdamW([p]) for p in params]
    refs = [oracle.AdamW([v], chunk) for v in values]
    scaler = optim.GradScaler('cuda', init_scale=4., growth_interval=2)
    scaler.scale(torch.zeros(1, device=device))
    assert len(optimizers) > optim.MAX_FOUND
    scale, tracker = 4., 0
    for step, bad in enumerate((None, 6, None)):
        grads = [oracle.gaussian((33,), 700 + 10 * step + k, 1e-2) + .5
                 for k in range(10)]
        if bad is not None:
            grads[bad][3] = float('nan')
        give(params, [(33, 0)] * 10, grads, device)
        for k, (optimizer, ref) in enumerate(zip(optimizers, refs)):
            scaler.step(optimizer)
            assert ref.step([grads[k]], scale) == (k == bad)
        scaler.update()
        scale, tracker = oracle.scaler_update(
            scale, tracker, bad is not None, interval=2)
        assert scaler.get_scale() == scale
        assert scaler._get_growth_tracker() == tracker
        for k, (optimizer, ref) in enumerate(zip(optimizers, refs)):
            assert_tensors(optimizer, [params[k]], ref, (step, k))
            assert optimizer.found_inf_scalar().item() == 0
    assert (scale, tracker) == (2., 1)
    assert [r.state.step for r in refs] == [3] * 6 + [2] + [3] * 3


@pytest.mark.gpu
def test_gradient_stats_of_a_module(device, chunk):
    model = TwoLayers().to(device)
    model(oracle.gaussian((4, 5), 77).to(device)).square().sum().backward()
    model.second.bias.grad = None       # a parameter without a gradient
    got = optim.gradient_stats(model)
    want = oracle.grad_stats(
        [p.grad.cpu() for p in model.parameters() if p.grad is not None],
        chunk)
    assert set(got) == set(optim.STATS_KEYS)
    for key, value in got.items():
        assert torch.equal(value.cpu(), want[key.split('/')[1]]), key


class TwoLayers(torch.nn.Module):

    def __init__(self):
        super().__init__()
        generator = torch.Generator().manual_seed(7)
        self.first = torch.nn.Linear(5, 7)
        self.second = torch.nn.Linear(7, 3)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=generator) * .3)

    def forward(self, x):
        return self.second(torch.tanh(self.first(x)))


@pytest.mark.gpu
def test_under_the_stock_scaler_and_under_ours(device, chunk):
    """Five steps, the third overflows: the parameters are the same under
    torch.amp.GradScaler and under ours, and the oracle's from the same
    gradients"""
    inputs = [oracle.gaussian((4, 5), 50 + k) for k in range(5)]
    weights = [1., 1., 3e38, 1., 1.]
    runs = {}
    for name, scaler_type in (('stock', torch.amp.GradScaler),
                              ('ours', optim.GradScaler)):
        model = TwoLayers().to(device)
        params = list(model.parameters())
        optimizer = optim.AdamW(params, lr=1e-2)
        scaler = scaler_type('cuda', init_scale=SCALE, growth_interval=2)
        ref = oracle.AdamW([p.detach().cpu() for p in params], chunk, lr=1e-2)
        scale, tracker, scales = SCALE, 0, []
        for k, x in enumerate(inputs):
            optimizer.zero_grad()
            loss = model(x.to(device)).square().sum() * weights[k]
            scaler.scale(loss).backward()
            grads = [p.grad.cpu() for p in params]
            scaler.step(optimizer)
            scaler.update()
            found = ref.step(grads, scale)
            assert found == (k == 2)
            scale, tracker = oracle.scaler_update(
                scale, tracker, found, interval=2)
            assert scaler.get_scale() == scale
            assert scaler._get_growth_tracker() == tracker
            scales.append(scale)
            for p, want in zip(params, ref.params):
                assert torch.equal(p.detach().cpu(), want), (name, k)
        assert scales == [SCALE, 2 * SCALE, SCALE, SCALE, 2 * SCALE]
        assert optimizer._state[0].item() == 4
        runs[name] = [p.detach().cpu() for p in params]
        assert scaler.state_dict().keys() == \
            torch.amp.GradScaler('cuda').state_dict().keys()
    for one, other in zip(runs['stock'], runs['ours']):
        assert torch.equal(one, other)


@pytest.mark.gpu
def test_three_replays_of_one_graph_equal_three_eager_steps(
        device, chunk, per_launch):
    """Statistics, update and scaler update captured in one graph; the second
    replay has an inf and is skipped. Two runs of the same steps are
    bit-identical."""
    count = 2 * per_launch + 10
    table = sizes(chunk, per_launch)[:count]
    values = parameters(chunk, per_launch)[:count]

    def grads_of(step):
        if step == 2:
            return planted(chunk, per_launch, float('inf'))[:count]
        return gradients(chunk, per_launch, step, torch.float32)[:count]

    def fresh():
        params = leaves(device, table, values)
        give(params, table, grads_of(0), device)
        optimizer = optim.AdamW(params, clip=1e-2)
        scaler = optim.GradScaler('cuda', init_scale=4., growth_interval=2)
        scaler.scale(torch.zeros(1, device=device))
        return params, optimizer, scaler

    def one_step(optimizer, scaler):
        scaler.step(optimizer)
        scaler.update()

    def copy_in(params, step):
        with torch.no_grad():
            for p, g in zip(params, grads_of(step)):
                p.grad.copy_(g)

    def snapshot(params, optimizer, scaler):
        return [t.clone() for p in params for t in (
            p.detach(), optimizer.state[p]['exp_avg'],
            optimizer.state[p]['exp_avg_sq'])] + [
            optimizer._state.clone(), optimizer._stats.clone(),
            scaler._scale.clone(), scaler._growth_tracker.clone()]

    def eager_run():
        params, optimizer, scaler = fresh()
        out = []
        for step in range(4):
            copy_in(params, step)
            one_step(optimizer, scaler)
            out.append(snapshot(params, optimizer, scaler))
        return out

    eager = eager_run()
    again = eager_run()
    for one, other in zip(eager, again):
        assert all(torch.equal(a, b) for a, b in zip(one, other))

    # step 0 eagerly (it allocates the state), then one graph for steps 1 .. 3
    params, optimizer, scaler = fresh()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        one_step(optimizer, scaler)
    torch.cuda.current_stream(device).wait_stream(side)
    first = snapshot(params, optimizer, scaler)
    assert all(torch.equal(a, b) for a, b in zip(first, eager[0]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step(optimizer, scaler)
    # (capturing runs nothing)
    assert all(torch.equal(a, b) for a, b in zip(
        snapshot(params, optimizer, scaler), first))
    for step in range(1, 4):
        copy_in(params, step)
        graph.replay()
        torch.cuda.synchronize(device)
        got = snapshot(params, optimizer, scaler)
        assert all(torch.equal(a, b) for a, b in zip(got, eager[step])), step
    # steps 0, 1, 3 were taken, step 2 was skipped and backed the scale off
    assert optimizer._state[0].item() == 3
    assert scaler.get_scale() == 4.


@pytest.mark.gpu
def test_state_dict_round_trips_with_torch_on_the_device(device, chunk,
                                                         per_launch):
    table = sizes(chunk, per_launch)[:9]
    values = parameters(chunk, per_launch)[:9]
    params = leaves(device, table, values)
    ours = optim.AdamW(params)
    ref = oracle.AdamW(values, chunk)
    for step in range(2):
        grads = gradients(chunk, per_launch, step, torch.float32)[:9]
        give(params, table, grads, device)
        ours.step()
        ref.step(grads)
    saved = ours.state_dict()
    assert all(set(s) == {'step', 'exp_avg', 'exp_avg_sq'}
               for s in saved['state'].values())
    assert all(float(s['step']) == 2 for s in saved['state'].values())
    # ours -> torch's -> ours, then one more step equals the oracle's third
    copies = [p.detach().clone().requires_grad_(True) for p in params]
    theirs = torch.optim.AdamW(
        copies, lr=2e-4, betas=(.8, .99), eps=1e-9, weight_decay=1e-2)
    theirs.load_state_dict(saved)
    again = optim.AdamW(copies)
    again.load_state_dict(theirs.state_dict())
    assert again._state.cpu().tolist() == [2., ref.state.b1pow,
                                           ref.state.b2pow]
    grads = gradients(chunk, per_launch, 2, torch.float32)[:9]
    give(copies, [(n, 0) for n, _ in table], grads, device)
    again.step()
    ref.step(grads)
    assert_tensors(again, copies, ref, 'reloaded')


@pytest.mark.gpu
def test_bad_arguments_change_nothing_on_the_device(device, chunk):
    library = _lib.lib()
    tensors = {name: torch.full((chunk + 3,), value, device=device)
               for name, value in (('p', 1.), ('m', 2.), ('v', 3.),
                                   ('g', 4.))}
    stats = torch.full((_lib.OPTIM_STATS,), 5., device=device)
    state = torch.tensor([1., .8, .99], dtype=torch.float64, device=device)
    workspace = torch.zeros(1 << 16, dtype=torch.uint8, device=device)

    def pointers(*values):
        return (ctypes.c_void_p * len(values))(*values)

    def longs(*values):
        return (ctypes.c_longlong * len(values))(*values)

    def ints(*values):
        return (ctypes.c_int * len(values))(*values)

    at = {name: t.data_ptr() for name, t in tensors.items()}

    def both(**changes):
        v = dict(dict(p=pointers(at['p'], at['p']),
                      m=pointers(at['m'], at['m']),
                      v=pointers(at['v'], at['v']),
                      g=pointers(at['g'], at['g']),
                      numel=longs(chunk + 3, 5), dtype=ints(0, 0)), **changes)
        return (library.pm_optim_grad_stats(
            v['g'], v['numel'], v['dtype'], 2, None, None, -1., .8, .99,
            state.data_ptr(), stats.data_ptr(), workspace.data_ptr(),
            workspace.numel(), _lib.stream()),
            library.pm_optim_adamw_step(
                v['p'], v['m'], v['v'], v['g'], v['numel'], v['dtype'], 2,
                stats.data_ptr(), state.data_ptr(), 2e-4, .8, .99, 1e-9, 1e-2,
                _lib.stream()))

    with torch.cuda.device(device):
        assert both(g=pointers(at['g'], None)) == (-1, -1)
        assert both(numel=longs(chunk + 3, 0)) == (-1, -1)
        assert both(numel=longs(chunk + 3, -5)) == (-1, -1)
        assert both(dtype=ints(0, 3)) == (-1, -1)
        assert both(p=pointers(at['p'], None)) == (0, -1)
    torch.cuda.synchronize(device)
    for name, value in (('p', 1.), ('m', 2.), ('v', 3.), ('g', 4.)):
        assert (tensors[name] == value).all()
    # (the one statistics pass that was well formed advanced the state)
    assert state.cpu().tolist() == [2., .8 * .8, .99 * .99]
    # a parameter that is not fp32 never reaches the library
    with pytest.raises(ValueError, match='fp32'):
        optim.AdamW([torch.zeros(4, device=device, dtype=torch.float16)])
