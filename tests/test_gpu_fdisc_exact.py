"""The conv layers of the FARGAN discriminator bit for bit: integer inputs,
weights, biases and upstream gradients in [-4, 4]. A pre-activation is a sum
of at most 18 * 9 products of at most 16 plus a bias, a weight or bias
gradient a sum over at most a few thousand pixels: every partial sum is an
integer below 2^24, so every order of summation gives the same fp32 value and
forward, gx, gW and gb are `torch.equal` to the float64 oracle
(tests/fdisc_oracle.py), the fixed-order reduction of the partials included.

  x      the embedding channels' weights are zero: the conv on the maps alone
         (gW is compared in the maps' channels);
  table  only the embedding channels' weights are nonzero and the (F, 2)
         table of sin and cos is replaced by integers (the `table` argument):
         the embedding's indexing and its zero padding at all four borders.

The activation of a case is the table's where it keeps integers (ReLU). The
sigmoid of the last layer does not (no format holds e^-z exactly): its case
runs here with activation 'none', which is exact, and with the sigmoid within
the gate in tests/test_gpu_fdisc.py.
"""
import pytest
import torch

from promonet_amd.model import discriminator

import fdisc_oracle as oracle

pytestmark = pytest.mark.gpu
NAMES = list(oracle.CASES)


def integer_case(name, which):
    channels, out_channels, bins, frames, dilation, activation = \
        oracle.CASES[name]
    generator = torch.Generator().manual_seed(
        11 + NAMES.index(name) + 100 * (which == 'table'))
    x = oracle.integers(
        (oracle.BATCH, channels, bins, frames), generator)
    weight = oracle.integers((out_channels, channels + 2, 3, 3), generator)
    if which == 'x':
        weight[:, channels:] = 0.
        table = None
    else:
        weight[:, :channels] = 0.
        table = oracle.integers((bins, 2), generator)
    bias = oracle.integers((out_channels,), generator)
    upstream = oracle.integers(
        (oracle.BATCH, out_channels, bins, frames), generator)
    if activation == 'sigmoid':
        activation = 'none'
    return x, weight, bias, upstream, table, dilation, activation


@pytest.mark.parametrize('which', ['x', 'table'])
@pytest.mark.parametrize('name', NAMES)
def test_integers_are_exact(device, name, which):
    x, weight, bias, upstream, table, dilation, activation = \
        integer_case(name, which)
    y = oracle.layer(x, weight, bias, dilation, activation, table=table)
    if activation == 'relu':
        assert (y > 0).any() and (y == 0).any()
    want = (y,) + oracle.layer_backward(
        x, weight, y, upstream, dilation, activation, table=table)
    assert all(v.abs().max() < 2 ** 24 for v in want)
    leaves = [t.to(device).requires_grad_(True) for t in (x, weight, bias)]
    got = discriminator.frequency_conv(
        *leaves, dilation, activation,
        # (without a table the embedding meets zero weights: 0 x sin = 0)
        table=None if table is None else table.to(device))
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
