"""FARGAN streaming latency and throughput (run on the GPU box):

  step   B = 1, one frame per call, per kernel mode and weight storage:
         median of STEPS calls after warm-up (each call synchronised), in
         us per frame, and the real-time factor against the 11.6 ms a
         256-sample hop lasts at 22.05 kHz;
  chunks B = 32 x 861 frames (config 5) streamed in chunks of 1, 8, 32 and
         128 frames with carried state, against one forward() in the same
         run.

Writes profiles/fargan_stream/bench.json.
    python scripts/bench_fargan_stream.py
"""
import json
import os
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import promonet_amd  # noqa: E402

HOP_MS = 256 / 22050 * 1e3
STEPS = int(os.environ.get('STEPS', 500))
device = torch.device('cuda:0')


def inputs(batch, frames, seed):
    gen = torch.Generator().manual_seed(seed)
    features = torch.randn(batch, 114, frames, generator=gen) * .5
    features[:, -1] = 40. + 360. * torch.rand(batch, frames, generator=gen)
    g = torch.randn(batch, 258, generator=gen) * .5
    return features.to(device), g.to(device)


def build(dtype):
    torch.manual_seed(0)
    model = promonet_amd.model.FARGAN(113, 258)
    model.weight_dtype = dtype
    return model.to(device).eval()


results = {'hop_ms': HOP_MS, 'step': {}, 'chunks': {}}
with torch.inference_mode():
    for dtype in ('fp32', 'mixed', 'f16'):
        model = build(dtype)
        features, g = inputs(1, 64, 1)
        for mode in (1, 2):
            model.kernel_mode = mode
            previous, states = None, None
            times = []
            for i in range(STEPS + 50):
                torch.cuda.synchronize()
                start = time.perf_counter()
                _, previous, states = model.step(
                    features[..., i % 64], g, previous, states)
                torch.cuda.synchronize()
                if i >= 50:
                    times.append(time.perf_counter() - start)
            us = statistics.median(times) * 1e6
            results['step'][f'{dtype}_mode{mode}'] = {
                'us_per_frame': us, 'p90_us': sorted(times)[
                    int(.9 * len(times))] * 1e6,
                'realtime_factor': HOP_MS * 1e3 / us}
            print(dtype, 'mode', mode, results['step'][f'{dtype}_mode{mode}'],
                  flush=True)

        model.kernel_mode = 0
        features, g = inputs(32, 861, 2)
        model(features[..., :8], g[..., None], None)
        entry = {}
        for name, chunk in (('forward', None), ('chunk1', 1), ('chunk8', 8),
                            ('chunk32', 32), ('chunk128', 128)):
            best = None
            for _ in range(2):
                torch.cuda.synchronize()
                start = time.perf_counter()
                if chunk is None:
                    model(features, g[..., None], None)
                else:
                    previous, states = None, None
                    for t in range(0, 861, chunk):
                        _, previous, states = model.stream(
                            features[..., t:t + chunk], g, previous, states)
                torch.cuda.synchronize()
                seconds = time.perf_counter() - start
                best = seconds if best is None else min(best, seconds)
            entry[name] = {'ms': best * 1e3}
        for name in entry:
            entry[name]['vs_forward'] = entry[name]['ms'] / entry['forward']['ms']
        results['chunks'][f'{dtype}_b32_t861'] = entry
        print(dtype, 'b32 x 861', entry, flush=True)

out = ROOT / 'profiles' / 'fargan_stream' / 'bench.json'
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(json.dumps(results, indent=1) + '\n')
print(json.dumps(results))
