"""The conv core that the family oracles share (tests/conv_oracle.py:
conv_forward, conv_adjoint) against torch's conv2d and autograd in float64, at
the smallest shape that has everything at once: both strides, a dilation, both
paddings, a kernel that is not square, and an input whose last window stops
short of the padded edge (on the width); and that neither hook of the adjoint
is silently ignored.
"""
import torch

import conv_oracle
from conv_checks import close

BATCH, CHANNELS, OUT_CHANNELS = 2, 3, 2
KERNEL, STRIDE, DILATION, PADDING = (3, 5), (2, 3), (2, 1), (2, 2)
HEIGHT, WIDTH = 7, 11
# (7 + 4 - 4 - 1) // 2 + 1 = 4 rows, (11 + 4 - 4 - 1) // 3 + 1 = 4 columns
OUT = tuple((size + 2 * p - d * (k - 1) - 1) // s + 1 for size, p, d, k, s in
            zip((HEIGHT, WIDTH), PADDING, DILATION, KERNEL, STRIDE))


def taps():
    for kh in range(KERNEL[0]):
        for kw in range(KERNEL[1]):
            first = kh * DILATION[0], kw * DILATION[1]
            yield (kh, kw) + tuple(
                slice(start, start + (count - 1) * stride + 1, stride)
                for start, count, stride in zip(first, OUT, STRIDE))


def case():
    generator = torch.Generator().manual_seed(0)
    x = torch.randn(BATCH, CHANNELS, HEIGHT, WIDTH, generator=generator,
                    dtype=torch.float64)
    weight = torch.randn(OUT_CHANNELS, CHANNELS, *KERNEL, generator=generator,
                         dtype=torch.float64)
    gz = torch.randn(BATCH, OUT_CHANNELS, *OUT, generator=generator,
                     dtype=torch.float64)
    source = torch.nn.functional.pad(
        x, (PADDING[1], PADDING[1], PADDING[0], PADDING[0]))
    return x, weight, gz, source


def inside(spread):
    """The gradient in x of the gradient in the padded source"""
    return spread[:, :, PADDING[0]:PADDING[0] + HEIGHT,
                  PADDING[1]:PADDING[1] + WIDTH]


def test_the_last_window_stops_short_of_the_padded_edge():
    """... on the width (the last padded column is read by no tap); on the
    height the four windows of five rows at stride 2 end on the edge"""
    assert OUT == (4, 4)
    ends = [(count - 1) * s + d * (k - 1) + 1 for d, k, s, count in zip(
        DILATION, KERNEL, STRIDE, OUT)]
    assert ends[0] == HEIGHT + 2 * PADDING[0]
    assert ends[1] == WIDTH + 2 * PADDING[1] - 1


def test_the_core_equals_conv2d_and_autograd_in_float64():
    x, weight, gz, source = case()
    leaf = x.clone().requires_grad_(True)
    leaf_weight = weight.clone().requires_grad_(True)
    want = torch.nn.functional.conv2d(
        leaf, leaf_weight, None, STRIDE, PADDING, DILATION)
    want.backward(gz)
    z = conv_oracle.conv_forward(source, weight, taps())
    assert z.shape == want.shape and close(z, want.detach())
    spread, grad_weight = conv_oracle.conv_adjoint(source, weight, gz, taps())
    assert close(inside(spread), leaf.grad)
    assert close(grad_weight, leaf_weight.grad)
    # the padding takes what the windows scatter there, and only x is kept
    assert spread.shape == source.shape and not torch.equal(
        spread.sum(), inside(spread).sum())


def test_a_tap_that_does_not_scatter_changes_gx_alone():
    _, weight, gz, source = case()
    spread, grad_weight = conv_oracle.conv_adjoint(source, weight, gz, taps())
    for dropped in ((0, 0), (1, 2), (2, 4)):
        other, same = conv_oracle.conv_adjoint(
            source, weight, gz, taps(),
            scatters=lambda kh, kw: (kh, kw) != dropped)
        assert torch.equal(same, grad_weight)
        assert not close(inside(other), inside(spread))
        # what is missing is that tap's term
        kh, kw = dropped
        only, _ = conv_oracle.conv_adjoint(
            source, weight, gz, taps(),
            scatters=lambda a, b: (a, b) == (kh, kw))
        assert close(other + only, spread)


def test_another_gz_for_the_weight_changes_gw_alone():
    _, weight, gz, source = case()
    spread, grad_weight = conv_oracle.conv_adjoint(source, weight, gz, taps())
    kept = gz.clone()
    kept[..., -1] = 0.
    same, other = conv_oracle.conv_adjoint(
        source, weight, gz, taps(), gz_of_weight=kept)
    assert torch.equal(same, spread)
    assert not close(other, grad_weight)
    _, wanted = conv_oracle.conv_adjoint(source, weight, kept, taps())
    assert torch.equal(other, wanted)
