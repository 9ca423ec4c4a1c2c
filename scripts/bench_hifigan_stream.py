"""Latency of HiFi-GAN streaming, and what a reduced lookahead
costs in accuracy. Writes one JSON object (--out; default
profiles/hifigan_stream/bench.json).

Latency: the wall time of one steady-state push, host clock around a call
that ends in a device synchronise, batch 1, default operand type; chunks of
8, 16, 32 and 64 frames, lookahead 13 and 0, eager and graph=True:
  stream          `Generator.packed_stream` (the nn~ call: unpack, feature
                  preparation, window kernel, forward of the window, emit
                  kernel)
  vocoder stream  `HiFiGAN.open_stream` on prepared channels-last features
Interleaved in the same rounds, the calls they are to be read against:
  packed(chunk)   packed_inference(graph=True) on the chunk's frames alone -
                  the nn~ call whose chunks do not join
  packed(window)  packed_inference(graph=True) on as many frames as the
                  stream's window holds (13 + lookahead + chunk): the same
                  forward without the two streaming launches
  vocoder forward(window, eager)  the same for the eager vocoder stream
  forward(861)    one eager forward of a 10 s utterance
One group of variants per chunk size; every variant is warmed until its
graphs exist; a round times every variant of the group once, the median over
--rounds rounds is reported, with the 10th and 90th percentile.

Deviation: for lookahead 0 ... 13, the max-abs difference between the
streamed audio (chunks of 8) and the full forward, at random-init scale and
with the output conv rescaled so that the audio peaks at 0.5 (the trained
scale of tests/test_gpu_model.py::test_precision_at_trained_scale).

    python scripts/bench_hifigan_stream.py [--rounds 200] [--out FILE]
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'oracle'))
import promonet_amd  # noqa: E402
import restatement as oracle  # noqa: E402

CHUNKS = (8, 16, 32, 64)
LOOKAHEADS = (13, 0)
LEFT = 13
FULL = 861


def make_model(state, device):
    model = promonet_amd.model.Generator()
    model.load_state_dict(state)
    return model.to(device).eval()


def packed_input(model, frames, device, seed):
    inputs = [t.to(device) for t in oracle.synthetic_inputs(1, frames, seed)]
    with torch.inference_mode():
        return model.pack_features(
            inputs[0], inputs[1][:, None], inputs[2][:, None],
            *inputs[3:]).clone()


def timed(call, device):
    torch.cuda.synchronize(device)
    start = time.perf_counter()
    call()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - start) * 1e3


def summary(samples):
    ordered = sorted(samples)
    return {'ms': statistics.median(ordered),
            'p10_ms': ordered[len(ordered) // 10],
            'p90_ms': ordered[len(ordered) * 9 // 10]}


def latency(model, device, rounds, warmup):
    """One group of variants per chunk size (a Generator keeps 8 packed
    graphs: a group captures 3), each group interleaved with itself"""
    vocoder = model.model
    full = packed_input(model, FULL, device, 7)
    out = {}
    for chunk in CHUNKS:
        x = packed_input(model, chunk, device, chunk)
        variants = {
            f'forward({FULL})': lambda: model.packed_inference(full),
            f'packed(chunk {chunk})':
                lambda: model.packed_inference(x, graph=True)}
        with torch.inference_mode():
            unpacked = [t.contiguous() for t in model.unpack_features(x)]
            features = model._features(*unpacked[:4], channels_last=True)
            g = model.prepare_global_features(*unpacked[4:])
        for lookahead in LOOKAHEADS:
            frames = LEFT + lookahead + chunk
            window = packed_input(model, frames, device, chunk + 100)
            variants[f'packed(window {frames})'] = \
                lambda w=window: model.packed_inference(w, graph=True)
            with torch.inference_mode():
                window_cl = model._features(
                    *[t.contiguous()
                      for t in model.unpack_features(window)[:4]],
                    channels_last=True)
            variants[f'vocoder forward(window {frames}, eager)'] = \
                lambda w=window_cl: vocoder.forward_channels_last(w, g)
            for graph in (False, True):
                how = 'graph' if graph else 'eager'
                stream = model.packed_stream(lookahead=lookahead, graph=graph)
                variants[f'stream(chunk {chunk}, lookahead {lookahead}, '
                         f'{how})'] = lambda s=stream: s.push(x)
                stream = vocoder.open_stream(g, 1, lookahead, graph)
                variants[f'vocoder stream(chunk {chunk}, lookahead '
                         f'{lookahead}, {how})'] = \
                    lambda s=stream: s.push(features, channels_last=True)
        samples = {name: [] for name in variants}
        with torch.inference_mode():
            for number in range(warmup + rounds):
                for name, call in variants.items():
                    ms = timed(call, device)
                    if number >= warmup:
                        samples[name].append(ms)
        for name, values in samples.items():
            key = name if name not in out else f'{name} [chunk {chunk}]'
            out[key] = summary(values)
    return out


def deviation(state, device):
    """max-abs |streamed - full| per lookahead, chunks of 8 over 120 frames"""
    inputs = oracle.synthetic_inputs(2, 120, seed=99)
    with torch.inference_mode():
        peak = oracle.generator_forward(*inputs, state).abs().max()
    trained = dict(state)
    trained['model.model.5.weight'] = state['model.model.5.weight'] * (
        math.atanh(.5) / math.atanh(float(peak)))
    inputs = [t.to(device) for t in inputs]
    out = {}
    for name, weights in (('random_init', state), ('trained_scale', trained)):
        model = make_model(weights, device)
        with torch.inference_mode():
            full = model(*inputs, None)
            rows = {}
            for lookahead in range(14):
                stream = model.open_stream(*inputs[4:], lookahead=lookahead)
                audio = [
                    stream.push(*[t[..., s:s + 8] for t in inputs[:4]])
                    for s in range(0, 120, 8)]
                audio.append(stream.finish())
                rows[lookahead] = (
                    torch.cat(audio, dim=-1) - full).abs().max().item()
        out[name] = {'audio_peak': full.abs().max().item(),
                     'max_abs_by_lookahead': rows}
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=200)
    parser.add_argument('--warmup', type=int, default=20)
    parser.add_argument(
        '--out', default=str(ROOT / 'profiles/hifigan_stream/bench.json'))
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_hifigan_stream.py needs a GPU')
    device = torch.device('cuda:0')
    state = oracle.random_state(seed=0)
    state['pitch_distribution'] = promonet_amd.load.pitch_distribution()
    model = make_model(state, device)
    result = {
        'compute_dtype': promonet_amd.COMPUTE_DTYPE,
        'batch': 1, 'rounds': args.rounds, 'warmup': args.warmup,
        'hop_ms': 1e3 * promonet_amd.HOPSIZE / promonet_amd.SAMPLE_RATE,
        'latency': latency(model, device, args.rounds, args.warmup),
        'reduced_lookahead': deviation(state, device)}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
