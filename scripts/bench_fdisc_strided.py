"""The five strided conv stacks of the FARGAN discriminator (n_fft 128 ...
2048) on the device beside the same formula on torch's own device ops, in one
run (run on the GPU box):

  hip       promonet_amd.model.discriminator: weight_norm and
            frequency_conv(stride=), forward, and forward + backward (the
            gradients in the input map and in every weight_g / weight_v / bias
            under a random upstream gradient at the logits and at each of the
            five maps, as the adversarial and the feature-matching losses
            give);
  torch     the reference's formula on torch device ops in fp32
            (FrequencyPositionalEmbedding's cat, torch._weight_norm, conv2d,
            ReLU in place / sigmoid), forward, and forward + backward through
            autograd;
  autocast  the same under torch.autocast('cuda'), fp16 convs: how the
            reference trains these stacks (promonet/train/core.py:220, :262);
  copy      a device copy moving the bytes the hip conv kernels read and
            write, from the shapes, the floor of a memory-bound pass. Forward:
            per layer the input map read and the output map written. Backward:
            per layer the upstream gradient and the saved output read twice
            (once for gx, once for gW and gb), the saved input read and gx
            written.

The maps are those of 256 x 4096 samples: n_fft / 2 + 1 bins, hop n_fft / 4.
The paths are interleaved round by round; device time between events, median
of ROUNDS rounds of CALLS calls after a warm-up of every shape. No pass mark.

Prints one JSON line and writes profiles/fdisc/bench_strided.json (or
--output).
    python scripts/bench_fdisc_strided.py [--resolution 2048]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from promonet_amd.model import discriminator  # noqa: E402
from disc_timing import ROUNDS, timed  # noqa: E402

BATCH, SAMPLES = 256, 4096
MATRIX_FP32 = 155e12        # the fp32 matrix rate the ratios are quoted against


def hip_layer(x, g, v, bias, stride, last):
    return discriminator.frequency_conv(
        x, discriminator.weight_norm(g, v), bias, 1,
        'sigmoid' if last else 'relu', stride=stride)


def torch_layer(x, g, v, bias, stride, last):
    bins = x.size(2)
    args = torch.arange(
        0, bins, dtype=x.dtype, device=x.device) * torch.pi * 2 / bins
    cos = torch.cos(args).reshape(1, 1, -1, 1)
    sin = torch.sin(args).reshape(1, 1, -1, 1)
    zeros = torch.zeros_like(x[:, 0:1, :, :])
    y = torch.nn.functional.conv2d(
        torch.cat((x, zeros + sin, zeros + cos), dim=1),
        torch._weight_norm(v, g, 0), bias, stride=(stride, 1), padding=(1, 1))
    return torch.sigmoid(y) if last else torch.relu_(y)


def autocast_layer(*arguments):
    with torch.autocast('cuda'):
        return torch_layer(*arguments)


def run(layer, x, parameters):
    outputs = []
    for g, v, bias, stride in parameters:
        x = layer(x, g, v, bias, stride, v.shape[0] == 1)
        outputs.append(x)
    return outputs


def geometry(parameters, batch, bins, frames):
    """[(input pixels, output pixels, channels, out_channels)] a layer"""
    out = []
    for _, v, _, stride in parameters:
        after = (bins - 1) // stride + 1
        out.append((batch * bins * frames, batch * after * frames,
                    v.shape[1] - 2, v.shape[0]))
        bins = after
    return out


def moved_bytes(layers):
    forward = backward = 0
    for pixels, out_pixels, channels, out_channels in layers:
        forward += 4 * (pixels * channels + out_pixels * out_channels)
        backward += 4 * (4 * out_pixels * out_channels + 2 * pixels * channels)
    return forward, forward + backward


def flops(parameters, layers):
    """Forward; the backward (gx and gW) is twice that"""
    return sum(2 * v[0].numel() * v.shape[0] * out_pixels
               for (_, v, _, _), (_, out_pixels, _, _) in
               zip(parameters, layers))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output',
        default=str(ROOT / 'profiles' / 'fdisc' / 'bench_strided.json'))
    parser.add_argument('--calls', type=int, default=3)
    parser.add_argument(
        '--resolution', type=int, action='append',
        choices=discriminator.RESOLUTIONS[1:],
        help='an n_fft to measure (repeatable); all five by default')
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fdisc_strided.py needs the GPU')
    device = torch.device('cuda:0')
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'batch': BATCH, 'samples': SAMPLES, 'matrix_fp32': MATRIX_FP32,
               'cases': {}}
    generator = torch.Generator(device).manual_seed(0)
    paths = {'hip': hip_layer, 'torch': torch_layer,
             'autocast': autocast_layer}
    for n_fft in args.resolution or discriminator.RESOLUTIONS[1:]:
        torch.manual_seed(n_fft)
        module = discriminator.DiscriminatorMagFree(
            [n_fft, n_fft // 4, n_fft], strided=True).to(device)
        parameters = [(layer[1].weight_g, layer[1].weight_v, layer[1].bias,
                       layer[1].stride) for layer in module.layers]
        bins, frames = n_fft // 2 + 1, 1 + SAMPLES // (n_fft // 4)
        layers = geometry(parameters, BATCH, bins, frames)
        x = 20. * torch.randn(BATCH, 1, bins, frames, device=device,
                              generator=generator) - 40.
        x.requires_grad_(True)
        leaves = [x] + [p for entry in parameters for p in entry[:3]]
        # one upstream gradient per output, in each path's own memory order
        # and dtype (as a loss on the maps returns it)
        with torch.no_grad():
            upstreams = {layer: [] for layer in paths.values()}
            values = [torch.randn(o.shape, device=device, generator=generator)
                      for o in run(hip_layer, x, parameters)]
            for layer in paths.values():
                for o, value in zip(run(layer, x, parameters), values):
                    upstreams[layer].append(torch.empty_like(o).copy_(value))
            del values

        def both(layer):
            return torch.autograd.grad(
                run(layer, x, parameters), leaves, upstreams[layer])

        copies = {}
        for name, count in zip(('forward', 'forward_backward'),
                               moved_bytes(layers)):
            source = torch.empty(
                count // 8, dtype=torch.float32, device=device)
            copies[name] = (source, torch.empty_like(source), count)
        forward = {f'{name}_forward': (
            lambda layer=layer: run(layer, x, parameters))
            for name, layer in paths.items()}
        forward['copy_forward'] = lambda: copies['forward'][1].copy_(
            copies['forward'][0])
        with torch.no_grad():
            stages = timed(forward, args.calls)
        backward = {f'{name}_forward_backward': (
            lambda layer=layer: both(layer)) for name, layer in paths.items()}
        backward['copy_forward_backward'] = \
            lambda: copies['forward_backward'][1].copy_(
                copies['forward_backward'][0])
        stages.update(timed(backward, args.calls))
        stages['bytes_forward'] = copies['forward'][2]
        stages['bytes_forward_backward'] = copies['forward_backward'][2]
        del copies
        work = flops(parameters, layers)
        stages['flop_forward'] = work
        stages['share_of_matrix_fp32_forward'] = work / (
            stages['hip_forward']['median_us'] * 1e-6) / MATRIX_FP32
        stages['share_of_matrix_fp32_forward_backward'] = 3 * work / (
            stages['hip_forward_backward']['median_us'] * 1e-6) / MATRIX_FP32
        stages['input_shape'] = [BATCH, 1, bins, frames]
        stages['layers'] = [[c, o, s] for (_, v, _, s), (_, _, c, o) in
                            zip(parameters, layers)]
        ours, theirs = both(hip_layer), both(torch_layer)
        stages['gradient_relative_l2'] = max(
            ((a - b).norm() / b.norm()).item() for a, b in zip(ours, theirs))
        with torch.no_grad():
            stages['output_max_abs_difference'] = max(
                (a - b).abs().max().item() for a, b in zip(
                    run(hip_layer, x, parameters),
                    run(torch_layer, x, parameters)))
        results['cases'][f'n_fft {n_fft}'] = stages
        print(json.dumps({f'n_fft {n_fft}': stages}), flush=True)
        del upstreams, ours, theirs, x, leaves, module, parameters
        torch.cuda.empty_cache()
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
