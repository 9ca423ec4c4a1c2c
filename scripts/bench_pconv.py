"""The conv stack of the multi-period discriminator on the device beside the
same formula on torch's own device ops, in one run (run on the GPU box):

  hip       promonet_amd.model.discriminator: weight_norm, period_fold_conv
            and period_conv, forward, and forward + backward (the gradients in
            the audio and in every weight_g / weight_v / bias under a random
            upstream gradient at every map, as the adversarial and the
            feature-matching losses give);
  torch     the reference's formula on torch device ops in fp32 (pad, view,
            torch._weight_norm, conv2d, leaky_relu), forward, and forward +
            backward through autograd;
  autocast  the same under torch.autocast('cuda'), which is what the
            reference trains with: the convs in 16-bit operands;
  copy      a device copy moving the bytes the hip conv kernels read and
            write, from the shapes, the floor of a memory-bound pass.
            Forward: per layer the input map and the weight read and the
            output map written. Backward: per layer the upstream gradient and
            the saved output read twice (once for gx, once for gW and gb), the
            saved input and the weight read, gx and the partials of gW
            written.

Cases, at the training shape of 64 x 16384 samples: one DiscriminatorP(2)
stack, the five stacks of the default configuration together, and the (1024,
1024, 5, 1) layer of period 2 alone. The paths are interleaved round by
round; device time between events, median of ROUNDS rounds of CALLS calls
after a warm-up of every shape. No pass mark.

Prints one JSON line and writes profiles/pconv/bench.json (or --output).
    python scripts/bench_pconv.py
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from promonet_amd import _lib  # noqa: E402
from promonet_amd.model import discriminator  # noqa: E402
from disc_timing import ROUNDS, timed  # noqa: E402

BATCH, SAMPLES = 64, 16384
SLOPE = 0.1
MATRIX_FP32 = 155e12        # the fp32 matrix rate the ratios are quoted against


def hip_stack(x, convs, fold):
    """Every map of the layers `convs` on x: the audio (fold: the period) or
    a map"""
    outputs = []
    for conv in convs:
        weight = discriminator.weight_norm(conv.weight_g, conv.weight_v)
        slope = 1. if weight.shape[0] == 1 else SLOPE
        if weight.shape[1] == 1 and fold:
            x = discriminator.period_fold_conv(
                x, weight, conv.bias, fold, slope)
        else:
            x = discriminator.period_conv(
                x, weight, conv.bias, conv.stride, slope)
        outputs.append(x)
    return outputs


def torch_stack(x, convs, fold):
    outputs = []
    if fold:
        batch, channels, samples = x.shape
        if samples % fold:
            x = torch.nn.functional.pad(
                x, (0, fold - samples % fold), 'reflect')
        x = x.view(batch, channels, -1, fold)
    for conv in convs:
        kernel = conv.weight_v.shape[2]
        x = torch.nn.functional.conv2d(
            x, torch._weight_norm(conv.weight_v, conv.weight_g, 0), conv.bias,
            stride=(conv.stride, 1), padding=((kernel - 1) // 2, 0))
        if conv.weight_v.shape[0] != 1:
            x = torch.nn.functional.leaky_relu(x, SLOPE)
        outputs.append(x)
    return outputs


def autocast_stack(x, convs, fold):
    with torch.autocast('cuda'):
        return torch_stack(x, convs, fold)


def run(stack, members):
    """[(x, convs, fold)] -> every map of every member"""
    return [y for member in members for y in stack(*member)]


def costs(members):
    """(bytes forward, bytes forward + backward, flop forward) from the
    shapes"""
    library = _lib.lib()
    forward = backward = flop = 0
    for x, convs, fold in members:
        batch, height, period = x.shape[0], -(-x.shape[-1] // fold) \
            if fold else x.shape[2], fold or x.shape[3]
        for conv in convs:
            out_channels, channels, kernel, _ = conv.weight_v.shape
            out_height = (height - 1) // conv.stride + 1
            pixels = batch * height * period
            out_pixels = batch * out_height * period
            weights = conv.weight_v.numel()
            forward += 4 * (pixels * channels + out_pixels * out_channels +
                            weights)
            backward += 4 * (4 * out_pixels * out_channels +
                             2 * pixels * channels + weights) + \
                library.pm_pconv_workspace_bytes(
                    batch, channels, out_channels, height, period, kernel,
                    conv.stride)
            flop += 2 * weights * out_pixels
            height = out_height
    return forward, forward + backward, flop


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'pconv' / 'bench.json'))
    parser.add_argument('--calls', type=int, default=3)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pconv.py needs the GPU')
    device = torch.device('cuda:0')
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'batch': BATCH, 'samples': SAMPLES,
               'matrix_fp32': MATRIX_FP32, 'cases': {}}
    torch.manual_seed(0)
    stacks = [discriminator.DiscriminatorP(period).to(device)
              for period in discriminator.PERIODS]
    generator = torch.Generator(device).manual_seed(0)
    audio = .1 * torch.randn(
        BATCH, 1, SAMPLES, device=device, generator=generator)

    def layers(module):
        return list(module.convs) + [module.conv_post]

    height = -(-SAMPLES // 2)
    for _ in range(4):
        height = (height - 1) // 3 + 1
    cases = (
        ('DiscriminatorP(2) stack', [(audio, layers(stacks[0]), 2)]),
        ('the five stacks',
         [(audio, layers(stack), stack.period) for stack in stacks]),
        ('layer (1024, 1024, 5, 1), period 2',
         [(torch.randn(BATCH, 1024, height, 2, device=device,
                       generator=generator),
           [stacks[0].convs[4]], 0)]))
    paths = {'hip': hip_stack, 'torch': torch_stack,
             'autocast': autocast_stack}
    for case, members in cases:
        members = [(x.clone().requires_grad_(True), convs, fold)
                   for x, convs, fold in members]
        leaves = [x for x, _, _ in members] + [
            p for _, convs, _ in members for conv in convs
            for p in (conv.weight_g, conv.weight_v, conv.bias)]
        # one upstream gradient per map, in each path's own memory order and
        # dtype (as a loss on the maps returns it)
        with torch.no_grad():
            maps = {name: run(stack, members)
                    for name, stack in paths.items()}
            upstreams = {name: [] for name in paths}
            for index, ours in enumerate(maps['hip']):
                values = torch.randn(
                    ours.shape, device=device, generator=generator)
                for name in paths:
                    upstreams[name].append(
                        torch.empty_like(maps[name][index]).copy_(values))
            differences = {
                name: max(((a - b.float()).norm() / a.norm()).item()
                          for a, b in zip(maps['torch'], maps[name]))
                for name in ('hip', 'autocast')}
            del maps

        def both(name):
            return torch.autograd.grad(
                run(paths[name], members), leaves, upstreams[name])

        bytes_forward, bytes_both, flop = costs(members)
        copies = {}
        for name, count in (('forward', bytes_forward),
                            ('forward_backward', bytes_both)):
            source = torch.empty(
                count // 8, dtype=torch.float32, device=device)
            copies[name] = (source, torch.empty_like(source))
        with torch.no_grad():
            functions = {
                f'{name}_forward': (lambda s=stack: run(s, members))
                for name, stack in paths.items()}
            functions['copy_forward'] = lambda: copies['forward'][1].copy_(
                copies['forward'][0])
            stages = timed(functions, args.calls)
        functions = {f'{name}_forward_backward': (lambda n=name: both(n))
                     for name in paths}
        functions['copy_forward_backward'] = \
            lambda: copies['forward_backward'][1].copy_(
                copies['forward_backward'][0])
        stages.update(timed(functions, args.calls))
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
        stages['input_shapes'] = [list(x.shape) for x, _, _ in members]
        stages['output_relative_l2_against_torch_fp32'] = differences
        theirs = both('torch')
        stages['gradient_relative_l2_against_torch_fp32'] = {
            name: max(((a.float() - b).norm() / b.norm()).item()
                      for a, b in zip(both(name), theirs))
            for name in ('hip', 'autocast')}
        results['cases'][case] = stages
        print(case, json.dumps(stages), file=sys.stderr, flush=True)
        del upstreams, theirs, members, leaves
        torch.cuda.empty_cache()
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
