"""The strided, wider conv layers of the FARGAN discriminator bit for bit:
integer inputs, weights, biases and upstream gradients in [-4, 4]
(fdisc_strided_oracle.integer_case). A pre-activation or an input gradient is
a sum of at most 258 * 9 products of at most 16, a weight or bias gradient a
sum over at most a few thousand pixels: every partial sum is an integer below
2^24 (tests/test_cpu_fdisc_strided.py asserts it), so every order of summation
gives the same fp32 value and forward, gx, gW and gb are `torch.equal` to the
float64 oracle, the fixed-order reduction of the partials included.

  x      the embedding channels' weights are zero: the conv on the maps alone
         (gW is compared in the maps' channels);
  table  only the embedding channels' weights are nonzero and the (F, 2)
         table of sin and cos is replaced by integers (the `table` argument):
         the embedding's row 2 f' + kf - 1 and its zero padding at all four
         borders.

A sigmoid case runs here with activation 'none', which is exact, and with the
sigmoid within the gate in tests/test_gpu_fdisc_strided.py.
"""
import pytest
import torch

from promonet_amd.model import discriminator

import fdisc_strided_oracle as oracle

pytestmark = pytest.mark.gpu
NAMES = list(oracle.CASES)


@pytest.mark.parametrize('which', ['x', 'table'])
@pytest.mark.parametrize('name', NAMES)
def test_integers_are_exact(device, name, which):
    x, weight, bias, upstream, table, stride, activation = \
        oracle.integer_case(name, which)
    y = oracle.layer(x, weight, bias, stride, activation, table=table)
    want = (y,) + oracle.layer_backward(
        x, weight, y, upstream, stride, activation, table=table)
    leaves = [t.to(device).requires_grad_(True) for t in (x, weight, bias)]
    got = discriminator.frequency_conv(
        *leaves, 1, activation,
        # (without a table the embedding meets zero weights: 0 x sin = 0)
        table=None if table is None else table.to(device), stride=stride)
    assert got.shape == y.shape
    got.backward(upstream.to(device))
    channels = x.shape[1]
    for label, mine, theirs in zip(
            oracle.QUANTITIES, (got, *(leaf.grad for leaf in leaves)), want):
        mine = mine.detach().cpu().double()
        if label == 'gW' and which == 'x':
            # (the weight gradient of the embedding channels is a sum of sines:
            # it is exact under the integer table)
            mine, theirs = mine[:, :channels], theirs[:, :channels]
        assert torch.equal(mine, theirs), label
