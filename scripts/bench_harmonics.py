"""Harmonic analysis on the device, stage by stage, beside the CPU oracle on
the same host (run on the GPU box):

  device  the stages of `preprocess.harmonics.from_audio` (high-pass, STFT
          magnitude, one observation, one Viterbi decode, the whole call) on
          1 x 10 s and 32 x 10 s: device time between events, median of
          ROUNDS rounds of CALLS calls;
  oracle  tests/harmonics_oracle.py on ONE 10 s recording (float64 biquad
          and STFT, fp32 observation, numpy Viterbi): wall time of one call
          each. A batch costs the oracle 32 times that.

Prints one JSON line and writes profiles/harmonics/bench.json (or --output).
    python scripts/bench_harmonics.py
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
import promonet_amd  # noqa: E402
from promonet_amd import viterbi  # noqa: E402
from promonet_amd.preprocess import harmonics  # noqa: E402
import harmonics_oracle as oracle  # noqa: E402

ROUNDS = 5


def device_time(function, calls):
    """Median / min / max microseconds per call over ROUNDS rounds"""
    function()
    torch.cuda.synchronize()
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    rounds = []
    for _ in range(ROUNDS):
        start.record()
        for _ in range(calls):
            function()
        end.record()
        end.synchronize()
        rounds.append(start.elapsed_time(end) * 1e3 / calls)
    return {'median_us': statistics.median(rounds), 'min_us': min(rounds),
            'max_us': max(rounds), 'calls_per_round': calls}


def wall(function):
    begin = time.perf_counter()
    result = function()
    return result, (time.perf_counter() - begin) * 1e6


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--output',
        default=str(ROOT / 'profiles' / 'harmonics' / 'bench.json'))
    parser.add_argument('--seconds', type=float, default=10.)
    parser.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_harmonics.py needs the GPU')
    device = torch.device('cuda:0')
    torch.set_num_threads(16)
    samples = int(args.seconds * promonet_amd.SAMPLE_RATE)
    voice, _ = oracle.synthetic_voice(samples)
    results = {'device': torch.cuda.get_device_name(0),
               'seconds': args.seconds, 'samples': samples,
               'frames': samples // promonet_amd.HOPSIZE,
               'host_threads': torch.get_num_threads(), 'device_stages': {}}
    cutoff = 1.33 * promonet_amd.FMIN
    rate = promonet_amd.SAMPLE_RATE
    for batch in args.batches:
        audio = torch.from_numpy(voice)[None].repeat(batch, 1).to(device)
        lengths = [samples] * batch
        filtered = harmonics.highpass(audio, rate, cutoff)
        frames, frequencies, counts = harmonics.magnitude(
            filtered, lengths, rate, promonet_amd.FMIN)
        transition, initial = harmonics.decoder_model(frequencies)
        observed, _ = harmonics.observation(frames, frequencies)
        calls = 4 if batch == 1 else 2
        stages = {
            'highpass': device_time(
                lambda: harmonics.highpass(audio, rate, cutoff), calls),
            'stft': device_time(
                lambda: harmonics.magnitude(
                    filtered, lengths, rate, promonet_amd.FMIN), calls),
            'observation': device_time(
                lambda: harmonics.observation(frames, frequencies), calls),
            'viterbi': device_time(
                lambda: viterbi.from_probabilities(
                    observed, counts, transition, initial, True), calls),
            'from_audio': device_time(
                lambda: harmonics.from_audio(audio, lengths=lengths), calls)}
        stages['viterbi_us_per_step'] = \
            stages['viterbi']['median_us'] / results['frames']
        stages['band_floats'] = transition.band.numel()
        results['device_stages'][f'{batch} x {args.seconds:g} s'] = stages

    filtered, t_highpass = wall(
        lambda: oracle.biquad(voice).astype(np.float32))
    (features, _, _), t_stft = wall(lambda: oracle.stft(filtered))
    freqs, _ = oracle.frequencies()
    features = features.to(torch.float32)
    (observed, _), t_observation = wall(
        lambda: oracle.observation(features, freqs))
    transition, initial = oracle.decoder_model(freqs)
    with np.errstate(divide='ignore'):
        log_transition = torch.log(transition).numpy()
        log_initial = torch.log(initial).numpy()
    _, t_viterbi = wall(lambda: oracle.viterbi(
        observed.numpy(), log_transition, log_initial))
    _, t_whole = wall(lambda: oracle.from_audio(voice))
    results['oracle_one_recording_us'] = {
        'highpass': t_highpass, 'stft': t_stft, 'observation': t_observation,
        'viterbi': t_viterbi, 'from_audio': t_whole}
    print(json.dumps(results), flush=True)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    output.write_text(json.dumps(results, indent=1) + '\n')


if __name__ == '__main__':
    main()
