"""The conv stacks of the complex multi-band and the multi-resolution
discriminators on the device beside the same formula on torch's own device
ops, in one run (run on the GPU box):

  hip     promonet_amd.model.discriminator: weight_norm and band_conv,
          forward, and forward + backward (the gradients in the input map and
          in every weight_g / weight_v / bias under a random upstream gradient
          at every map, as the adversarial and the feature-matching losses
          give);
  torch   the reference's formula on torch device ops in fp32
          (torch._weight_norm, conv2d, leaky_relu, torch.cat), forward, and
          forward + backward through autograd;
  copy    a device copy moving the bytes the hip conv kernels read and write,
          from the shapes, the floor of a memory-bound pass. Forward: per
          layer the input map read and the output map written. Backward: per
          layer the upstream gradient and the saved output read twice (once
          for gx, once for gW and gb), the saved input read and gx written.

Cases, at the training shape of 64 x 16384 samples: the CMB stack on 64
frames x 513 bins in the default bands, one (32, 32, 9, 2) layer of its widest
band, and the R stack at (1024, 120, 600) on 513 bins x 136 frames. The three
paths are interleaved round by round; device time between events, median of
ROUNDS rounds of CALLS calls after a warm-up of every shape. No pass mark.

Prints one JSON line and writes profiles/dconv/bench.json (or --output).
    python scripts/bench_dconv.py
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

BATCH, FRAMES, BINS = 64, 64, 513
RESOLUTION = (1024, 120, 600)
R_FRAMES = 1 + (16384 + 2 * ((1024 - 120) // 2) - 1024) // 120
MATRIX_FP32 = 155e12        # the fp32 matrix rate the ratios are quoted against


def hip_layer(x, conv, slope):
    return discriminator.band_conv(
        x, discriminator.weight_norm(conv.weight_g, conv.weight_v), conv.bias,
        conv.stride, slope)


def torch_layer(x, conv, slope):
    kernel_width = conv.weight_v.shape[3]
    y = torch.nn.functional.conv2d(
        x, torch._weight_norm(conv.weight_v, conv.weight_g, 0), conv.bias,
        stride=(1, conv.stride), padding=(1, (kernel_width - 1) // 2))
    return y if slope == 1. else torch.nn.functional.leaky_relu(y, slope)


def run(layer, inputs, chains, slope, post):
    """Every map: the chains' (one a band), then conv_post on their last
    maps joined on the width axis (post None: a chain alone)"""
    outputs, last = [], []
    for x, convs in zip(inputs, chains):
        for conv in convs:
            x = layer(x, conv, slope)
            outputs.append(x)
        last.append(x)
    if post is not None:
        outputs.append(layer(torch.cat(last, dim=-1), post, 1.))
    return outputs


def layer_costs(inputs, chains, post):
    """(bytes forward, bytes forward + backward, flop forward) from the
    shapes"""
    forward = backward = flop = 0
    widths = []
    for x, convs in zip(inputs, chains):
        batch, _, height, width = x.shape
        for conv in convs:
            out_channels, channels, _, kernel_width = conv.weight_v.shape
            out_width = (width - 1) // conv.stride + 1
            pixels, out_pixels = batch * height * width, \
                batch * height * out_width
            forward += 4 * (pixels * channels + out_pixels * out_channels)
            backward += 4 * (4 * out_pixels * out_channels +
                             2 * pixels * channels)
            flop += 2 * conv.weight_v.numel() * out_pixels
            width = out_width
        widths.append(width)
    if post is not None:
        pixels = batch * height * sum(widths)
        forward += 4 * pixels * 33
        backward += 4 * pixels * (4 + 64)
        flop += 2 * post.weight_v.numel() * pixels
    return forward, forward + backward, flop


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'dconv' / 'bench.json'))
    parser.add_argument('--calls', type=int, default=3)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dconv.py needs the GPU')
    device = torch.device('cuda:0')
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'batch': BATCH, 'matrix_fp32': MATRIX_FP32, 'cases': {}}
    torch.manual_seed(0)
    cmb = discriminator.DiscriminatorCMB().to(device)
    res = discriminator.DiscriminatorR(RESOLUTION).to(device)
    generator = torch.Generator(device).manual_seed(0)

    def magnitudes(*shape):
        return torch.randn(shape, device=device, generator=generator).abs()

    edges = discriminator.band_edges()
    spectrogram = magnitudes(BATCH, 1, FRAMES, BINS)
    widest = max(range(len(edges)), key=lambda i: edges[i][1] - edges[i][0])
    cases = (
        ('CMB stack',
         [spectrogram[..., low:high] for low, high in edges],
         [[layer[0] for layer in convs] for convs in cmb.band_convs],
         0.1, cmb.conv_post),
        ('CMB layer (32, 32, 9, 2), widest band',
         [torch.randn(BATCH, 32, FRAMES, edges[widest][1] - edges[widest][0],
                      device=device, generator=generator)],
         [[cmb.band_convs[widest][1][0]]], 0.1, None),
        ('R stack', [magnitudes(BATCH, 1, BINS, R_FRAMES)],
         [list(res.convs)], 0.2, res.conv_post))
    for case, inputs, chains, slope, post in cases:
        inputs = [x.clone().requires_grad_(True) for x in inputs]
        leaves = inputs + [
            p for convs in chains + ([[post]] if post is not None else [])
            for conv in convs
            for p in (conv.weight_g, conv.weight_v, conv.bias)]
        # one upstream gradient per map, in each path's own memory order (as
        # a loss on the maps returns it)
        with torch.no_grad():
            upstreams = {hip_layer: [], torch_layer: []}
            for ours, theirs in zip(
                    run(hip_layer, inputs, chains, slope, post),
                    run(torch_layer, inputs, chains, slope, post)):
                values = torch.randn(
                    ours.shape, device=device, generator=generator)
                upstreams[hip_layer].append(
                    torch.empty_like(ours).copy_(values))
                upstreams[torch_layer].append(
                    torch.empty_like(theirs).copy_(values))

        def both(layer):
            return torch.autograd.grad(
                run(layer, inputs, chains, slope, post), leaves,
                upstreams[layer])

        bytes_forward, bytes_both, flop = layer_costs(inputs, chains, post)
        copies = {}
        for name, count in (('forward', bytes_forward),
                            ('forward_backward', bytes_both)):
            source = torch.empty(
                count // 8, dtype=torch.float32, device=device)
            copies[name] = (source, torch.empty_like(source))
        with torch.no_grad():
            stages = timed({
                'hip_forward':
                    lambda: run(hip_layer, inputs, chains, slope, post),
                'torch_forward':
                    lambda: run(torch_layer, inputs, chains, slope, post),
                'copy_forward': lambda: copies['forward'][1].copy_(
                    copies['forward'][0])}, args.calls)
        stages.update(timed({
            'hip_forward_backward': lambda: both(hip_layer),
            'torch_forward_backward': lambda: both(torch_layer),
            'copy_forward_backward':
                lambda: copies['forward_backward'][1].copy_(
                    copies['forward_backward'][0])}, args.calls))
        del copies
        stages['bytes_forward'] = bytes_forward
        stages['bytes_forward_backward'] = bytes_both
        stages['flop_forward'] = flop
        stages['share_of_matrix_fp32_forward'] = flop / (
            stages['hip_forward']['median_us'] * 1e-6) / MATRIX_FP32
        stages['share_of_matrix_fp32_forward_backward'] = 3 * flop / (
            stages['hip_forward_backward']['median_us'] * 1e-6) / MATRIX_FP32
        stages['input_shapes'] = [list(x.shape) for x in inputs]
        ours, theirs = both(hip_layer), both(torch_layer)
        stages['gradient_relative_l2'] = max(
            ((a - b).norm() / b.norm()).item() for a, b in zip(ours, theirs))
        with torch.no_grad():
            stages['output_max_abs_difference'] = max(
                (a - b).abs().max().item() for a, b in zip(
                    run(hip_layer, inputs, chains, slope, post),
                    run(torch_layer, inputs, chains, slope, post)))
        results['cases'][case] = stages
        del upstreams, ours, theirs, inputs, leaves
        torch.cuda.empty_cache()
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
