"""The optimizer step on the device beside torch's own, in one run (run on the
GPU box). One step is what promonet/train/core.py:338-369 does after the
backward: the gradient statistics, scaler.step(optimizer), scaler.update().

  hip          promonet_amd.optim.AdamW under promonet_amd.optim.GradScaler:
               the statistics pass (which is also the inf check and the clip
               decision), the update pass, the scaler kernel; no host read;
  hip_graph    the same three captured in one graph and replayed;
  torch_fused  torch.optim.AdamW(fused=True) under torch.amp.GradScaler, and
               the statistics on torch ops: max and min of every gradient
               (two reductions a tensor), reduced once more on the device
               and read on the host once each, as the reference reads them.
               (The fused step writes the unscaled gradient back, so this
               path's gradients shrink from step to step; its time does not
               depend on their values.)
  torch_foreach  the same with foreach=True, whose scaler.step also reads
               found_inf on the host;
  copy         a device copy moving the bytes the hip path moves: 32 bytes
               an element (g, p, m, v read and p, m, v written by the update,
               g read once more by the statistics pass), the floor of a
               memory-bound pass.

The lists are the parameters of the library's own default Generator (HiFi-GAN)
and of its FARGAN, with random gradients standing for a backward pass. The
paths are interleaved round by round; device time between events, median of
ROUNDS rounds of --calls steps after a warm-up of every path.

Prints one JSON line and writes profiles/optim/bench.json (or --output).
    python scripts/bench_optim.py
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
import promonet_amd.optim  # noqa: E402

ROUNDS = 7
HYPER = dict(lr=2e-4, betas=(.8, .99), eps=1e-9, weight_decay=1e-2)
SCALE = 2. ** 16


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


def leaves(shapes, gradients, device):
    out = []
    for shape, gradient in zip(shapes, gradients):
        leaf = torch.zeros(shape, device=device).requires_grad_(True)
        leaf.grad = gradient.clone()
        out.append(leaf)
    return out


def torch_statistics(parameters):
    """The two figures the reference reads, on torch ops: a reduction a
    tensor, the maxima and the minima stacked and reduced on the device, and
    one host read for each of the two figures"""
    largest = torch.stack([p.grad.max() for p in parameters]).max()
    smallest = torch.stack([p.grad.min() for p in parameters]).min()
    return largest.item(), smallest.item()


def torch_path(parameters, **flags):
    optimizer = torch.optim.AdamW(parameters, **HYPER, **flags)
    scaler = torch.amp.GradScaler('cuda', init_scale=SCALE)
    scaler.scale(torch.zeros(1, device=parameters[0].device))

    def step():
        torch_statistics(parameters)
        scaler.step(optimizer)
        scaler.update()
    return step


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output', default=str(ROOT / 'profiles' / 'optim' / 'bench.json'))
    parser.add_argument('--calls', type=int, default=5)
    parser.add_argument('--note', action='append', default=[],
                        help='a remark to keep in the file (repeatable)')
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim.py needs the GPU')
    device = torch.device('cuda:0')
    library = promonet_amd._lib.lib()
    chunk = library.pm_optim_chunk()
    per_launch = library.pm_optim_entries_per_launch()
    results = {'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
               'chunk': chunk, 'entries_per_launch': per_launch, 'cases': {},
               'notes': list(args.note)}
    generator = torch.Generator(device).manual_seed(0)
    for model in ('hifigan', 'fargan'):
        promonet_amd.configure(MODEL=model)
        shapes = [p.shape for p in promonet_amd.model.Generator().parameters()]
        # gradients as a backward under the scale leaves them
        gradients = [
            torch.randn(shape, device=device, generator=generator) * 1e-3 *
            SCALE for shape in shapes]
        elements = sum(g.numel() for g in gradients)

        ours = leaves(shapes, gradients, device)
        optimizer = promonet_amd.optim.AdamW(ours, **HYPER)
        scaler = promonet_amd.optim.GradScaler('cuda', init_scale=SCALE)
        scaler.scale(torch.zeros(1, device=device))

        def hip():
            scaler.step(optimizer)
            scaler.update()

        replayed = leaves(shapes, gradients, device)
        graph_optimizer = promonet_amd.optim.AdamW(replayed, **HYPER)
        graph_scaler = promonet_amd.optim.GradScaler('cuda', init_scale=SCALE)
        graph_scaler.scale(torch.zeros(1, device=device))

        def hip_once():
            graph_scaler.step(graph_optimizer)
            graph_scaler.update()

        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            hip_once()
        torch.cuda.current_stream(device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hip_once()

        moved = 32 * elements
        source = torch.empty(moved // 8, dtype=torch.float32, device=device)
        target = torch.empty_like(source)
        stages = timed({
            'hip': hip,
            'hip_graph': graph.replay,
            'torch_fused': torch_path(
                leaves(shapes, gradients, device), fused=True),
            'torch_foreach': torch_path(
                leaves(shapes, gradients, device), foreach=True),
            'copy': lambda: target.copy_(source)}, args.calls)
        groups = sum(-(-g.numel() // chunk) for g in gradients)
        slices = -(-len(shapes) // per_launch)
        stages.update({
            'tensors': len(shapes), 'elements': elements,
            'bytes_moved': moved, 'workgroups_a_pass': groups,
            # the statistics slices and their final workgroup, the update
            # slices, the scaler
            'hip_launches': slices + 1 + slices + 1,
            'hip_over_copy': stages['hip_graph']['median_us'] /
            stages['copy']['median_us'],
            'hip_over_torch_fused': stages['hip_graph']['median_us'] /
            stages['torch_fused']['median_us']})
        if stages['hip_over_copy'] > 1.5:
            results['notes'].append(
                f'{model}: the replayed graph takes '
                f'{stages["hip_over_copy"]:.2f} x the copy of the same bytes '
                '(above 1.5 x: not tuned here, see DESIGN.md section 20)')
        results['cases'][model] = stages
        del ours, replayed, graph, source, target, gradients
        torch.cuda.empty_cache()
    promonet_amd.configure(MODEL='hifigan')
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
