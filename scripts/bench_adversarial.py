"""The adversarial generator losses on the device beside the same formulas on
torch's own device ops, in one run (run on the GPU box):

  hip     promonet_amd.loss.feature_matching + generator, forward, and
          forward + backward (the gradient by the fake maps and logits);
  torch   the reference's formula on torch device ops: per pair
          mean(|real.float().detach() - fake.float()|) added up, and per logit
          tensor mean((1 - x)^2) or mean(clamp(1 - x, min=0)), forward, and
          forward + backward through autograd;
  copy    a device copy moving the bytes the hip path reads and writes (the
          maps and logits read once forward; with the backward read once
          more and the gradients written), the floor of a memory-bound pass.

The lists are the feature maps of the reference's discriminators, recorded at
B = 1 by scripts/make_golden_adversarial.py (tests/golden/adversarial.pt) and
scaled to the reference's default BATCH_SIZE: 5 period + 3 resolution
discriminators with the hinge loss (config/baselines/vocos.py, 48 maps, 8
logit tensors) and 5 period + the complex multi-band discriminator with least
squares (the default configuration, 56 maps, 6 logit tensors), each with fp32
and f16 maps. The three paths are interleaved round by round; device time
between events, median of ROUNDS rounds of CALLS calls after a warm-up of
every shape.

Prints one JSON line and writes profiles/adversarial/bench.json (or --output).
    python scripts/bench_adversarial.py
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import promonet_amd  # noqa: E402

ROUNDS = 7
SETS = {'period+resolution, hinge': (('period', 'resolution'), True),
        'period+multiband, least squares': (('period', 'multiband'), False)}
MAX_ENTRIES = 64    # entries a launch (ADV_MAX_ENTRIES, pm_adv.h)


def torch_feature_matching(real_feature_maps, fake_feature_maps):
    loss = 0.
    for reals, fakes in zip(real_feature_maps, fake_feature_maps):
        for real, fake in zip(reals, fakes):
            loss = loss + torch.mean(
                torch.abs(real.float().detach() - fake.float()))
    return loss


def torch_generator(outputs, hinge):
    if hinge:
        return sum(torch.mean(torch.clamp(1. - o, min=0.)) for o in outputs)
    return sum(torch.mean((1. - o) ** 2.) for o in outputs)


def launches(maps, logits, sixteen_bit, hinge):
    """Kernel launches of both paths, counted from their op sequences (not
    traced). hip: one launch per 64 entries and the final pass, forward; one
    per 64 entries backward. torch, per map: sub, abs, mean, add (and two
    casts of 16-bit maps); backward the mean's expand-and-scale, abs's sign
    and product, the negation for the subtrahend (and a cast). Per logit
    tensor: rsub, pow or clamp, mean, add; backward the mean's scale, the
    pow's (pow, two products) or the clamp's mask, the negation."""
    def slices(count):
        return -(-count // MAX_ENTRIES)
    hip_forward = slices(maps) + 1 + slices(logits) + 1
    hip_backward = slices(maps) + slices(logits)
    torch_forward = maps * (4 + 2 * sixteen_bit) + logits * 4
    torch_backward = maps * (4 + sixteen_bit) + logits * (3 if hinge else 5)
    return {'hip_forward': hip_forward,
            'hip_forward_backward': hip_forward + hip_backward,
            'torch_forward': torch_forward,
            'torch_forward_backward': torch_forward + torch_backward}


def timed(functions, calls):
    """Interleaved: every round times each function once, `calls` calls"""
    for function in functions.values():
        function()
    torch.cuda.synchronize()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    rounds = {name: [] for name in functions}
    for _ in range(ROUNDS):
        for name, function in functions.items():
            start.record()
            for _ in range(calls):
                function()
            end.record()
            end.synchronize()
            rounds[name].append(start.elapsed_time(end) * 1e3 / calls)
    return {name: {'median_us': statistics.median(r), 'min_us': min(r),
                   'max_us': max(r), 'calls_per_round': calls}
            for name, r in rounds.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output',
        default=str(ROOT / 'profiles' / 'adversarial' / 'bench.json'))
    parser.add_argument('--batch', type=int, default=None,
                        help='default: the recorded BATCH_SIZE')
    parser.add_argument('--calls', type=int, default=3)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_adversarial.py needs the GPU')
    device = torch.device('cuda:0')
    golden = torch.load(ROOT / 'tests' / 'golden' / 'adversarial.pt')
    batch = args.batch or golden['batch_size']
    results = {'device': torch.cuda.get_device_name(0), 'batch': batch,
               'chunk_size': golden['chunk_size'], 'rounds': ROUNDS,
               'cases': {}}
    generator = torch.Generator(device).manual_seed(0)
    for name, (groups, hinge) in SETS.items():
        promonet_amd.configure(ADVERSARIAL_HINGE_LOSS=hinge)
        shapes = [[[batch] + shape[1:] for shape in maps]
                  for group in groups for maps in golden['shapes'][group]]
        for dtype, label in ((torch.float32, 'fp32'), (torch.float16, 'f16')):
            def randn(shape, requires_grad):
                return torch.randn(
                    shape, device=device, generator=generator).to(
                    dtype).requires_grad_(requires_grad)
            real = [[randn(s, False) for s in maps] for maps in shapes]
            fake = [[randn(s, True) for s in maps] for maps in shapes]
            logits = [randn((batch, maps[-1].numel() // batch), True)
                      for maps in fake]
            leaves = [m for maps in fake for m in maps] + logits
            elements = sum(m.numel() for maps in fake for m in maps)
            logit_elements = sum(l.numel() for l in logits)
            size = leaves[0].element_size()
            moved = {
                'forward': (2 * elements + logit_elements) * size,
                'forward_backward':
                    (5 * elements + 3 * logit_elements) * size}

            def hip_forward():
                return promonet_amd.loss.feature_matching(real, fake) + \
                    promonet_amd.loss.generator(logits)[0]

            def torch_forward():
                return torch_feature_matching(real, fake) + \
                    torch_generator(logits, hinge)

            copies = {}
            for case, count in moved.items():
                source = torch.empty(
                    count // 8, dtype=torch.float32, device=device)
                copies[case] = (source, torch.empty_like(source))
            with torch.no_grad():
                stages = timed({
                    'hip_forward': hip_forward,
                    'torch_forward': torch_forward,
                    'copy_forward': lambda: copies['forward'][1].copy_(
                        copies['forward'][0])}, args.calls)
            stages.update(timed({
                'hip_forward_backward': lambda: torch.autograd.grad(
                    hip_forward(), leaves),
                'torch_forward_backward': lambda: torch.autograd.grad(
                    torch_forward(), leaves),
                'copy_forward_backward':
                    lambda: copies['forward_backward'][1].copy_(
                        copies['forward_backward'][0])}, args.calls))
            del copies
            stages['bytes_forward'] = moved['forward']
            stages['bytes_forward_backward'] = moved['forward_backward']
            stages['maps'] = len(leaves) - len(logits)
            stages['logit_tensors'] = len(logits)
            stages['map_elements'] = elements
            stages['launches'] = launches(
                stages['maps'], len(logits), dtype != torch.float32, hinge)
            with torch.no_grad():
                ours, theirs = hip_forward(), torch_forward()
            stages['loss_hip'], stages['loss_torch'] = \
                ours.item(), theirs.item()
            ours = torch.autograd.grad(hip_forward(), leaves)
            theirs = torch.autograd.grad(torch_forward(), leaves)
            stages['gradient_relative_l2'] = max(
                ((a.float() - b.float()).norm() / b.float().norm()).item()
                for a, b in zip(ours, theirs))
            results['cases'][f'{name}, {label}'] = stages
            del real, fake, logits, leaves, ours, theirs
            torch.cuda.empty_cache()
    promonet_amd.configure(ADVERSARIAL_HINGE_LOSS=False)
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
