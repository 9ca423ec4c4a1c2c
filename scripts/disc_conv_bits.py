"""Digest of what the discriminator conv layers and the generator's Block conv
compute.

For every case of tests/fdisc_oracle.py (CASES), tests/dconv_oracle.py
(ALL_CASES), tests/pconv_oracle.py (ALL_CASES), tests/fdisc_strided_oracle.py
(CASES) and tests/gconv_oracle.py (CASES, at both SLOPES, without and with
the residual), on the oracles' seeded random inputs, generated on the CPU: one
line per output tensor (forward, gx, gW, gb) with its sha256. The kernels use
no float atomics, so two builds of the same arithmetic give the same lines,
and a change that claims to leave the arithmetic alone shows it by equal
listings from the two libraries, each in a process of its own. Hashes only;
needs a GPU. The cases are the oracles': the smallest that reach a second
tile, a partial last tile, a second gW partial and every kernel variant.

    PROMONET_HIP_LIB=<build>/libpromonet_hip.so python scripts/disc_conv_bits.py
"""
import hashlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import dconv_oracle                                         # noqa: E402
import fdisc_oracle                                         # noqa: E402
import fdisc_strided_oracle                                 # noqa: E402
import gconv_oracle                                         # noqa: E402
import pconv_oracle                                         # noqa: E402
from promonet_amd.model import discriminator, hifigan_train  # noqa: E402

DEVICE = torch.device('cuda', 0)


def frequency(name, x, weight, bias):
    _, _, _, _, dilation, activation = fdisc_oracle.CASES[name]
    return discriminator.frequency_conv(x, weight, bias, dilation, activation)


def band(name, x, weight, bias):
    _, _, _, stride, _, _, slope = dconv_oracle.ALL_CASES[name]
    return discriminator.band_conv(x, weight, bias, stride, slope)


def period(name, x, weight, bias):
    _, _, _, stride, slope = pconv_oracle.form_of(name)
    if name in pconv_oracle.FOLD_CASES:
        return discriminator.period_fold_conv(
            x, weight, bias, pconv_oracle.FOLD_CASES[name][1], slope)
    return discriminator.period_conv(x, weight, bias, stride, slope)


def strided(name, x, weight, bias):
    _, _, _, _, stride, activation = fdisc_strided_oracle.CASES[name]
    return discriminator.frequency_conv(
        x, weight, bias, 1, activation, stride=stride)


def show(name, tensor):
    data = tensor.detach().cpu().contiguous().numpy().tobytes()
    print(f'{name:44} {hashlib.sha256(data).hexdigest()}')


def lines(kind, oracle, names, layer):
    for name in names:
        x, weight, bias, upstream = (
            t.to(DEVICE) for t in oracle.inputs(name))
        x, weight, bias = (
            t.requires_grad_(True) for t in (x, weight, bias))
        y = layer(name, x, weight, bias)
        y.backward(upstream)
        for quantity, tensor in zip(
                oracle.QUANTITIES, (y, x.grad, weight.grad, bias.grad)):
            show(f'{kind} {name} {quantity}', tensor)


def block_lines():
    for name in gconv_oracle.CASES:
        dilation = gconv_oracle.CASES[name][2]
        for slope in gconv_oracle.SLOPES:
            for with_residual in (False, True):
                x, weight, bias, upstream, residual = (
                    t.to(DEVICE) for t in gconv_oracle.inputs(name))
                x, weight, bias = (
                    t.requires_grad_(True) for t in (x, weight, bias))
                y = hifigan_train.block_conv(
                    x, weight, bias, dilation, slope,
                    residual if with_residual else None)
                y.backward(upstream)
                kind = f'gconv {name} {slope:g}' + \
                    (' residual' if with_residual else '')
                for quantity, tensor in zip(
                        gconv_oracle.QUANTITIES,
                        (y, x.grad, weight.grad, bias.grad)):
                    show(f'{kind} {quantity}', tensor)


def main():
    lines('fdisc', fdisc_oracle, fdisc_oracle.CASES, frequency)
    lines('dconv', dconv_oracle, dconv_oracle.ALL_CASES, band)
    lines('pconv', pconv_oracle, pconv_oracle.ALL_CASES, period)
    lines('fstrided', fdisc_strided_oracle, fdisc_strided_oracle.CASES,
          strided)
    block_lines()


if __name__ == '__main__':
    main()
