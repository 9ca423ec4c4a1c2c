"""The generator's training path on the device beside the same composition on
torch's own device ops, in one run (run on the GPU box):

  hip       promonet_amd.model.hifigan_train: block_conv on the kernels of
            pm_gconv.h under ResidualBlock / HiFiGANTrainable, forward, and
            forward + backward (the gradients in the input and in every
            weight_g / weight_v / bias under a random upstream gradient);
  torch     the reference's formula on torch device ops in fp32
            (torch._weight_norm, leaky_relu, conv1d, conv_transpose1d),
            forward, and forward + backward through autograd;
  autocast  the same under torch.autocast('cuda'), which is what the
            reference trains with: the convs in 16-bit operands;
  copy      a device copy moving the bytes of the activations the hip conv
            kernels read and write, from the shapes, the floor of a
            memory-bound pass. Forward: per conv the input read and the output
            written, and the residual read by every second conv. Backward:
            per conv the upstream gradient and the saved input read twice
            (once for gx, once for gW and gb) and gx written.

Cases, at the training shape of 64 utterances x 64 frames: the ResidualBlock
of each of the four stages (256 channels x 512 frames ... 32 x 16384), the
whole HiFiGANTrainable, and every one of the 36 layer forms alone at its
stage's shape. The paths are interleaved round by round; device time between
events, median of ROUNDS rounds of CALLS calls after a warm-up of every shape.
No pass mark.

Prints one JSON line and writes profiles/hifigan_train/bench.json (or
--output).
    python scripts/bench_gconv.py
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import promonet_amd  # noqa: E402
from promonet_amd.model import hifigan_train  # noqa: E402
from disc_timing import ROUNDS, timed  # noqa: E402

BATCH, FRAMES = 64, 64
SLOPE = 0.1
MATRIX_FP32 = 157e12        # the fp32 matrix peak the shares are quoted against
functional = torch.nn.functional


def torch_conv(x, conv, dilation, residual=None):
    kernel = conv.weight_v.shape[2]
    y = functional.conv1d(
        functional.leaky_relu(x, SLOPE),
        torch._weight_norm(conv.weight_v, conv.weight_g, 0), conv.bias,
        dilation=dilation, padding=(kernel - 1) // 2 * dilation)
    return y if residual is None else y + residual


def torch_residual(module, x):
    total = None
    for block in module.model:
        y = x
        for c1, c2, d in zip(block.convs1, block.convs2, block.dilation):
            y = torch_conv(torch_conv(y, c1, d), c2, 1, y)
        total = y if total is None else total + y
    return total / len(module.model)


def torch_vocoder(module, x, g):
    x = functional.conv1d(
        x, module.input_feature_conv.weight, module.input_feature_conv.bias,
        padding=3)
    x = x + functional.conv1d(
        g, module.input_speaker_conv.weight, module.input_speaker_conv.bias)
    for index in range(module.stages):
        stage = module.model[str(index)]
        upsampler = stage.model['1']
        x = functional.conv_transpose1d(
            functional.leaky_relu(x, SLOPE),
            torch._weight_norm(upsampler.weight_v, upsampler.weight_g, 0),
            upsampler.bias, stride=stage.rate, padding=stage.padding)
        x = torch_residual(stage.model['2'], x)
    x = functional.conv1d(
        functional.leaky_relu(x, SLOPE),
        module.model[str(module.stages + 1)].weight, None, padding=3)
    return torch.tanh(x)


def autocast(function):
    def run(*args):
        with torch.autocast('cuda'):
            return function(*args)
    return run


def measure(paths, inputs, leaves, flop, bytes_forward, bytes_both, calls,
            generator):
    """The timings of one case. paths: {name: function of *inputs}"""
    device = inputs[0].device
    with torch.no_grad():
        outputs = {name: path(*inputs) for name, path in paths.items()}
        values = torch.randn(
            outputs['hip'].shape, device=device, generator=generator)
        upstreams = {name: torch.empty_like(out).copy_(values)
                     for name, out in outputs.items()}
        differences = {
            name: ((outputs['torch'] - outputs[name].float()).norm() /
                   outputs['torch'].norm()).item()
            for name in ('hip', 'autocast')}
        del outputs, values

    def both(name):
        return torch.autograd.grad(
            paths[name](*inputs), leaves, upstreams[name])

    copies = {}
    for name, count in (('forward', bytes_forward),
                        ('forward_backward', bytes_both)):
        source = torch.empty(count // 8, dtype=torch.float32, device=device)
        copies[name] = (source, torch.empty_like(source))
    with torch.no_grad():
        functions = {f'{name}_forward': (lambda p=path: p(*inputs))
                     for name, path in paths.items()}
        functions['copy_forward'] = lambda: copies['forward'][1].copy_(
            copies['forward'][0])
        stages = timed(functions, calls)
    functions = {f'{name}_forward_backward': (lambda n=name: both(n))
                 for name in paths}
    functions['copy_forward_backward'] = \
        lambda: copies['forward_backward'][1].copy_(
            copies['forward_backward'][0])
    stages.update(timed(functions, calls))
    del copies
    stages['bytes_forward'] = bytes_forward
    stages['bytes_forward_backward'] = bytes_both
    stages['flop_forward'] = flop
    for name in paths:
        stages[f'share_of_matrix_fp32_{name}_forward'] = flop / (
            stages[f'{name}_forward']['median_us'] * 1e-6) / MATRIX_FP32
        stages[f'share_of_matrix_fp32_{name}_forward_backward'] = \
            3 * flop / (stages[f'{name}_forward_backward']['median_us'] *
                        1e-6) / MATRIX_FP32
    stages['output_relative_l2_against_torch_fp32'] = differences
    theirs = both('torch')
    stages['gradient_relative_l2_against_torch_fp32'] = {
        name: max(((a.float() - b).norm() / b.norm()).item()
                  for a, b in zip(both(name), theirs))
        for name in ('hip', 'autocast')}
    return stages


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output',
        default=str(ROOT / 'profiles' / 'hifigan_train' / 'bench.json'))
    parser.add_argument('--calls', type=int, default=2)
    parser.add_argument('--no-forms', action='store_true',
                        help='leave the 36 single layers out')
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_gconv.py needs the GPU')
    device = torch.device('cuda:0')
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'batch': BATCH, 'frames': FRAMES, 'matrix_fp32': MATRIX_FP32,
               'cases': {}}
    torch.manual_seed(0)
    generator = torch.Generator(device).manual_seed(0)
    vocoder = hifigan_train.HiFiGANTrainable(113, 258).to(device)
    channels, frames, shapes = promonet_amd.HIFIGAN_UPSAMPLE_INITIAL_SIZE, \
        FRAMES, []
    for rate in promonet_amd.HIFIGAN_UPSAMPLE_RATES:
        channels, frames = channels // 2, frames * rate
        shapes.append((channels, frames))

    def record(case, stages):
        results['cases'][case] = stages
        print(case, json.dumps(stages), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    for index, (channels, frames) in enumerate(shapes):
        module = vocoder.model[str(index)].model['2']
        x = torch.randn(BATCH, channels, frames, device=device,
                        generator=generator).requires_grad_(True)
        convs = sum(2 * len(block.dilation) for block in module.model)
        flop = sum(2 * 2 * len(block.dilation) * channels * channels *
                   block.convs1[0].weight_v.shape[2] * BATCH * frames
                   for block in module.model)
        one = 4 * BATCH * channels * frames
        record(f'ResidualBlock({channels}) at {frames} frames', measure(
            {'hip': module, 'torch': lambda x, m=module: torch_residual(m, x),
             'autocast': autocast(lambda x, m=module: torch_residual(m, x))},
            (x,), [x] + list(module.parameters()), flop,
            one * (2 * convs + convs // 2),
            one * (2 * convs + convs // 2 + 5 * convs), args.calls,
            generator))
        del x

    x = torch.randn(BATCH, 113, FRAMES, device=device,
                    generator=generator).requires_grad_(True)
    g = torch.randn(BATCH, 258, 1, device=device,
                    generator=generator).requires_grad_(True)
    flop = sum(results['cases'][case]['flop_forward']
               for case in results['cases'])
    total = sum(results['cases'][case]['bytes_forward']
                for case in results['cases'])
    total_both = sum(results['cases'][case]['bytes_forward_backward']
                     for case in results['cases'])
    stages = measure(
        {'hip': vocoder, 'torch': lambda x, g: torch_vocoder(vocoder, x, g),
         'autocast': autocast(lambda x, g: torch_vocoder(vocoder, x, g))},
        (x, g), [x, g] + list(vocoder.parameters()), flop, total, total_both,
        args.calls, generator)
    stages['note'] = 'flop and bytes: the convs of the Blocks alone'
    record('HiFiGANTrainable', stages)
    del x, g

    if not args.no_forms:
        for channels, frames in shapes:
            for kernel in hifigan_train.KERNELS:
                conv = hifigan_train._Normed(
                    (channels, channels, kernel), channels,
                    channels * kernel).to(device)
                for dilation in hifigan_train.DILATIONS:
                    x = torch.randn(
                        BATCH, channels, frames, device=device,
                        generator=generator).requires_grad_(True)
                    one = 4 * BATCH * channels * frames
                    record(f'layer ({channels}, {kernel}, {dilation})', measure(
                        {'hip': lambda x, c=conv, d=dilation:
                            hifigan_train.block_conv(
                                x, c.weight(), c.bias, d, SLOPE),
                         'torch': lambda x, c=conv, d=dilation:
                            torch_conv(x, c, d),
                         'autocast': autocast(
                             lambda x, c=conv, d=dilation:
                             torch_conv(x, c, d))},
                        (x,), [x] + list(conv.parameters()),
                        2 * channels * channels * kernel * BATCH * frames,
                        2 * one, 7 * one, args.calls, generator))
                    del x
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
