"""The conv stack of the FARGAN discriminator on the device beside the same
formula on torch's own device ops, in one run (run on the GPU box):

  hip     promonet_amd.model.discriminator: weight_norm and frequency_conv,
          forward, and forward + backward (the gradients in the input map and
          in every weight_g / weight_v / bias under a random upstream gradient
          at the logits and at each of the five maps, as the adversarial and
          the feature-matching losses give);
  torch   the reference's formula on torch device ops in fp32
          (FrequencyPositionalEmbedding's cat, torch._weight_norm, conv2d,
          ReLU in place / sigmoid), forward, and forward + backward through
          autograd;
  copy    a device copy moving the bytes the hip conv kernels read and write,
          from the shapes, the floor of a memory-bound pass. Forward: per
          layer the input map read and the output map written. Backward: per
          layer the upstream gradient and the saved output read twice (once
          for gx, once for gW and gb), the saved input read and gx written.

Cases: the stack of n_fft = 64 (33 bins, hop 16: the one resolution whose
layers the kernels compute) and one of its 16 -> 16 layers alone, on the maps
of 256 x 4096 and 64 x 16384 samples. The three paths are interleaved round
by round; device time between events, median of ROUNDS rounds of CALLS calls
after a warm-up of every shape. No pass mark.

Prints one JSON line and writes profiles/fdisc/bench.json (or --output).
    python scripts/bench_fdisc.py
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

N_FFT, HOP = 64, 16
MATRIX_FP32 = 155e12        # the fp32 matrix rate the ratios are quoted against


def hip_layer(x, g, v, bias, dilation, last):
    return discriminator.frequency_conv(
        x, discriminator.weight_norm(g, v), bias, dilation,
        'sigmoid' if last else 'relu')


def torch_layer(x, g, v, bias, dilation, last):
    bins = x.size(2)
    args = torch.arange(
        0, bins, dtype=x.dtype, device=x.device) * torch.pi * 2 / bins
    cos = torch.cos(args).reshape(1, 1, -1, 1)
    sin = torch.sin(args).reshape(1, 1, -1, 1)
    zeros = torch.zeros_like(x[:, 0:1, :, :])
    y = torch.nn.functional.conv2d(
        torch.cat((x, zeros + sin, zeros + cos), dim=1),
        torch._weight_norm(v, g, 0), bias, dilation=(dilation, 1),
        padding=(dilation, 1))
    return torch.sigmoid(y) if last else torch.relu_(y)


def run(layer, x, parameters):
    outputs = []
    for index, (g, v, bias, dilation) in enumerate(parameters):
        x = layer(x, g, v, bias, dilation, v.shape[0] == 1)
        outputs.append(x)
    return outputs


def moved_bytes(parameters, pixels):
    forward = backward = 0
    for _, v, _, _ in parameters:
        out_channels, channels = v.shape[0], v.shape[1] - 2
        forward += 4 * pixels * (channels + out_channels)
        backward += 4 * pixels * (4 * out_channels + 2 * channels)
    return forward, forward + backward


def flops(parameters, pixels):
    """Forward; the backward (gx and gW) is twice that"""
    return sum(2 * v[0].numel() * v.shape[0] * pixels
               for _, v, _, _ in parameters)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'fdisc' / 'bench.json'))
    parser.add_argument('--calls', type=int, default=3)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fdisc.py needs the GPU')
    device = torch.device('cuda:0')
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'n_fft': N_FFT, 'hop': HOP, 'matrix_fp32': MATRIX_FP32,
               'cases': {}}
    torch.manual_seed(0)
    module = discriminator.DiscriminatorMagFree(
        [N_FFT, HOP, N_FFT]).to(device)
    stack = [(layer[1].weight_g, layer[1].weight_v, layer[1].bias,
              layer[1].dilation) for layer in module.layers]
    generator = torch.Generator(device).manual_seed(0)
    for batch, samples in ((256, 4096), (64, 16384)):
        bins, frames = N_FFT // 2 + 1, 1 + samples // HOP
        pixels = batch * bins * frames
        for case, parameters, channels in (
                ('stack', stack, 1), ('layer 16 -> 16', stack[2:3], 16)):
            x = torch.randn(batch, channels, bins, frames, device=device,
                            generator=generator)
            if channels == 1:
                x = 20. * x - 40.
            x.requires_grad_(True)
            leaves = [x] + [p for entry in parameters for p in entry[:3]]
            # one upstream gradient per output, in each path's own memory
            # order (as a loss on the maps returns it)
            with torch.no_grad():
                upstreams = {hip_layer: [], torch_layer: []}
                for o in run(hip_layer, x, parameters):
                    values = torch.randn(
                        o.shape, device=device, generator=generator)
                    upstreams[torch_layer].append(values)
                    upstreams[hip_layer].append(
                        torch.empty_like(o).copy_(values))

            def both(layer):
                return torch.autograd.grad(
                    run(layer, x, parameters), leaves, upstreams[layer])

            copies = {}
            for name, count in zip(('forward', 'forward_backward'),
                                   moved_bytes(parameters, pixels)):
                source = torch.empty(
                    count // 8, dtype=torch.float32, device=device)
                copies[name] = (source, torch.empty_like(source), count)
            with torch.no_grad():
                stages = timed({
                    'hip_forward': lambda: run(hip_layer, x, parameters),
                    'torch_forward': lambda: run(torch_layer, x, parameters),
                    'copy_forward': lambda: copies['forward'][1].copy_(
                        copies['forward'][0])}, args.calls)
            stages.update(timed({
                'hip_forward_backward': lambda: both(hip_layer),
                'torch_forward_backward': lambda: both(torch_layer),
                'copy_forward_backward':
                    lambda: copies['forward_backward'][1].copy_(
                        copies['forward_backward'][0])}, args.calls))
            stages['bytes_forward'] = copies['forward'][2]
            stages['bytes_forward_backward'] = copies['forward_backward'][2]
            del copies
            work = flops(parameters, pixels)
            stages['flop_forward'] = work
            stages['share_of_matrix_fp32_forward'] = work / (
                stages['hip_forward']['median_us'] * 1e-6) / MATRIX_FP32
            stages['share_of_matrix_fp32_forward_backward'] = 3 * work / (
                stages['hip_forward_backward']['median_us'] * 1e-6) / \
                MATRIX_FP32
            stages['map_shape'] = [batch, 16, bins, frames]
            ours, theirs = both(hip_layer), both(torch_layer)
            stages['gradient_relative_l2'] = max(
                ((a - b).norm() / b.norm()).item()
                for a, b in zip(ours, theirs))
            with torch.no_grad():
                stages['output_max_abs_difference'] = max(
                    (a - b).abs().max().item() for a, b in zip(
                        run(hip_layer, x, parameters),
                        run(torch_layer, x, parameters)))
            results['cases'][f'{case}, {batch} x {samples}'] = stages
            del upstreams, ours, theirs, x, leaves
            torch.cuda.empty_cache()
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
