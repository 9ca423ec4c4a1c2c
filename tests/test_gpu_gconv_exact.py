"""One conv of the generator's MRF Block on the device, exactly: integer
inputs, upstream gradients and residuals in [-4, 4], weights and biases in
[-2, 2], with slope 0.5 and slope 1. Every product is at most 8 in half-units
and an output sums at most K = 2816 of them: the largest partial sum is far
below 2^24; gx sums at most 2816 products of at most 8 and is halved exactly
under the slope; gW sums one product of at most 16 in half-units a pixel over
fewer than 2^11 pixels. So every sum is exact in fp32 in ANY order, the
fixed-order reduction of the partials included, and forward, gx, gW and gb
must be torch.equal to the float64 oracle (tests/gconv_oracle.py): no
tolerance.
"""
import pytest
import torch

from promonet_amd.model import hifigan_train

import gconv_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('slope', oracle.EXACT_SLOPES)
@pytest.mark.parametrize('name', oracle.EXACT_CASES)
def test_integers_are_exact(device, name, slope):
    want = oracle.truth(name, slope, exact=True)
    x = want['x']
    assert x.shape[0] * x.shape[2] < 2 ** 11
    # the gate has zeros to decide: x = 0 takes the slope
    assert (x == 0.).any() and (x > 0.).any() and (x < 0.).any()
    leaves = [want[key].to(device).requires_grad_(True)
              for key in ('x', 'weight', 'bias', 'residual')]
    got = hifigan_train.block_conv(
        *leaves[:3], oracle.CASES[name][2], slope, leaves[3])
    got.backward(want['upstream'].to(device))
    for label, mine, truth in (
            ('forward', got.detach(), want['forward_residual']),
            ('gx', leaves[0].grad, want['gx']),
            ('gW', leaves[1].grad, want['gW']),
            ('gb', leaves[2].grad, want['gb']),
            ('residual', leaves[3].grad, want['upstream'].double())):
        assert truth.dtype == torch.float64
        assert mine.shape == truth.shape, label
        assert torch.equal(mine.cpu().double(), truth), label
    plain = hifigan_train.block_conv(
        *(leaf.detach() for leaf in leaves[:3]), oracle.CASES[name][2], slope)
    assert torch.equal(plain.cpu().double(), want['forward'])
