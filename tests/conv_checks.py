"""The test bodies that the conv-layer families share
(tests/test_{cpu,gpu}_{fdisc,fdisc_strided,dconv,pconv,gconv}.py): a family's
test modules describe it once (Family) and their tests call these. Nothing
here is collected.
"""
import torch

from promonet_amd.model import discriminator

import conv_oracle


def close(got, want):
    """The project's float64 closeness"""
    return (got - want).abs().max() <= 1e-12 * want.abs().max()


class Family:
    """A family for the bodies below. `layer(case, x, weight, bias, rows)`
    calls the layer on the device (`rows`: the slice of the batch that x is);
    `truth(case)`, `figures(case, y, gx, gW, gb)` and `recorded(case)` default
    to the oracle's, a case being a name of its table."""

    def __init__(self, oracle, layer, truth=None, figures=None,
                 recorded=None, label=str):
        self.oracle, self.layer, self.label = oracle, layer, label
        self.truth = truth or oracle.truth
        self.figures = figures or oracle.figures
        self.recorded = recorded or (
            lambda case: oracle.FP32_RECORDED.get(case, ()))
        self.results = {}

    def forward_backward(self, device, case, rows=slice(None)):
        """(y, gx, gW, gb) of the case on the device, on the CPU"""
        want = self.truth(case)
        x = want['x'][rows].to(device).requires_grad_(True)
        weight = want['weight'].to(device).requires_grad_(True)
        bias = want['bias'].to(device).requires_grad_(True)
        y = self.layer(case, x, weight, bias, rows)
        y.backward(want['upstream'][rows].to(device))
        return tuple(
            t.detach().cpu() for t in (y, x.grad, weight.grad, bias.grad))

    def result(self, device, case):
        if case not in self.results:
            self.results[case] = self.forward_backward(device, case)
        return self.results[case]


###############################################################################
# On the device
###############################################################################


def a_layer_is_within_the_gate(family, device, case):
    oracle, want = family.oracle, family.truth(case)
    got = family.result(device, case)
    assert got[0].shape == want['forward'].shape
    assert got[1].shape == want['x'].shape
    figures = family.figures(case, *got)
    print(f'{family.label(case)}: device ' +
          ' '.join(f'{v:.3e}' for v in figures) + ' fp32 CPU recorded ' +
          ' '.join(f'{v:.3e}' for v in family.recorded(case)))
    for quantity, value in zip(oracle.QUANTITIES, figures):
        assert value < oracle.gate(quantity), (quantity, value)


def weight_norm_is_within_the_gate(oracle, device, shape):
    def run(g, v, upstream):
        leaf_g = g.to(device).requires_grad_(True)
        leaf_v = v.to(device).requires_grad_(True)
        w = discriminator.weight_norm(leaf_g, leaf_v)
        w.backward(upstream.to(device))
        return w.detach().cpu(), leaf_g.grad.cpu(), leaf_v.grad.cpu()

    figures = conv_oracle.weight_norm_figures(run, shape)
    print(f'{shape}: device ' + ' '.join(f'{v:.3e}' for v in figures))
    for value, limit in zip(figures, oracle.WEIGHT_NORM_GATES):
        assert value < limit, (value, limit)


def two_runs_are_bit_identical(family, device, case):
    first = family.result(device, case)
    second = family.forward_backward(device, case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def a_row_alone_equals_the_row_in_its_batch(family, device, case):
    whole = family.result(device, case)
    alone = family.forward_backward(device, case, slice(1, 2))
    assert torch.equal(alone[0], whole[0][1:2])
    assert torch.equal(alone[1], whole[1][1:2])


def forward_and_backward_capture_into_one_graph(family, device, case):
    want = family.truth(case)
    generator = torch.Generator().manual_seed(5)
    other = torch.randn(want['x'].shape, generator=generator)
    static = want['x'].to(device).requires_grad_(True)
    weight = want['weight'].to(device).requires_grad_(True)
    bias = want['bias'].to(device).requires_grad_(True)
    upstream = want['upstream'].to(device)

    def step():
        out = family.layer(case, static, weight, bias, slice(None))
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


def zero_input_gives_the_bias(family, device, case, slope):
    """... under the leaky activation of the slope"""
    want = family.truth(case)
    bias = want['bias'].to(device)
    y = family.layer(case, torch.zeros_like(want['x']).to(device),
                     want['weight'].to(device), bias, slice(None))
    expected = torch.where(bias > 0., bias, bias * slope)
    assert torch.equal(y, expected[None, :, None, None].expand_as(y))


def bf16_input_returns_a_bf16_gradient(family, device, case):
    want = family.truth(case)
    leaf = want['x'].to(device, torch.bfloat16).requires_grad_(True)
    arguments = [want[k].to(device) for k in ('weight', 'bias')]
    y = family.layer(case, leaf, *arguments, slice(None))
    assert y.dtype == torch.float32
    y.backward(want['upstream'].to(device))
    assert leaf.grad.dtype == torch.bfloat16 and leaf.grad.shape == leaf.shape
    exact = family.layer(
        case, leaf.detach().float(), *arguments, slice(None))
    assert torch.equal(y, exact)


def autocast_computes_in_fp32(family, device, case):
    want = family.truth(case)
    arguments = [want[k].to(device) for k in ('x', 'weight', 'bias')]
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = family.layer(case, *arguments, slice(None))
    assert y.dtype == torch.float32
    assert torch.equal(y, family.layer(case, *arguments, slice(None)))


###############################################################################
# Without a GPU: what the GPU tests rely on. `layer(x, weight, bias)` and
# `backward(x, weight, y, upstream)` are the oracle's layer of the case with
# a defect planted.
###############################################################################


def the_fragile_share_is_small(oracle, name):
    want = oracle.truth(name)
    share = want['fragile'].double().mean().item()
    print(f'{name}: fragile share {share:.1e}')
    assert share <= 1e-3, share
    assert not want['upstream'][want['fragile']].any()


def the_gates_come_from_the_reference_arithmetic_in_fp32(oracle, name):
    """4 x the largest recorded figure of the quantity over the table; the
    fp32 torch arithmetic itself, run here, stays inside the gates"""
    figures = oracle.fp32_figures(name)
    print(f'{name}: fp32 torch ' + ' '.join(f'{v:.3e}' for v in figures) +
          f' (recorded {oracle.FP32_RECORDED[name]})')
    for index, quantity in enumerate(oracle.QUANTITIES):
        assert figures[index] < oracle.gate(quantity)
        assert oracle.gate(quantity) == 4. * max(
            recorded[index] for recorded in oracle.FP32_RECORDED.values())


def the_weight_norm_gates_come_from_torch_in_fp32(oracle, shape):
    figures = oracle.weight_norm_fp32_figures(shape)
    print(f'{shape}: fp32 torch ' + ' '.join(f'{v:.3e}' for v in figures))
    for value, limit in zip(figures, oracle.WEIGHT_NORM_GATES):
        assert value < limit


def accepted(oracle, name, layer, backward):
    """Would the GPU tests pass this implementation of the case?"""
    want = oracle.truth(name)
    y = layer(want['x'], want['weight'], want['bias'])
    if y.shape != want['forward'].shape:
        return False
    gradients = backward(want['x'], want['weight'], y, want['upstream'])
    return all(value < oracle.gate(quantity) for quantity, value in zip(
        oracle.QUANTITIES, oracle.figures(name, y, *gradients)))
