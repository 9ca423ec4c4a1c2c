"""CPU restatement of the reference's `FARGAN.step` (model/fargan.py:65-131)
from an arbitrary recurrent state, built from oracle/restatement.py's
`fargan_subframe` / `fargan_weights`. Used by scripts/make_golden_fargan_step.py
(pinned there against the reference itself) and by the streaming tests."""
import torch
import torch.nn.functional as F

import restatement as oracle


def fargan_step(w, features, global_features, previous_samples, states):
    """features (B, 114) with the pitch period last, global_features (B, 258),
    previous_samples (B, 1, 512), states the reference's 4-tuple ->
    (signal (B, 256), previous_samples (B, 1, 512), states)."""
    batch = features.shape[0]
    period = torch.round(features[:, -1]).to(torch.long)        # :94
    x = torch.cat((features[:, :-1], global_features), dim=1)
    for i in range(3):                                          # :139-160
        x = torch.tanh(F.linear(x, w[f'cond{i}']))
    prev = previous_samples[:, 0]
    outs = []
    for sub in x.reshape(batch, 2 * oracle.FARGAN_SUBFRAME_SIZE,
                         oracle.FARGAN_SUBFRAMES).permute(2, 0, 1):
        out, states = oracle.fargan_subframe(w, sub, prev, period, states)
        outs.append(out)
        prev = torch.cat((prev[:, oracle.FARGAN_SUBFRAME_SIZE:], out), dim=1)
    return torch.cat(outs, dim=1), prev[:, None], tuple(states)


def fargan_stream(w, features, global_features, previous_samples, states):
    """`fargan_step` over the frames of features (B, 114, T) ->
    (signal (B, 1, 256 T), previous_samples, states)."""
    frames = []
    for frame in features.permute(2, 0, 1):
        out, previous_samples, states = fargan_step(
            w, frame, global_features, previous_samples, states)
        frames.append(out)
    return torch.cat(frames, dim=1)[:, None], previous_samples, states


def features(batch, frames, state, seed):
    """(B, 114, T) FARGAN input features (the pitch period in samples last)
    and (B, 258) global features from oracle.synthetic_inputs."""
    inputs = oracle.synthetic_inputs(batch, frames, seed=seed)
    x = oracle.prepare_features(
        *inputs[:4], state['pitch_distribution'],
        state['pitch_embedding.weight'], state['ppg_threshold'])
    period = oracle.SAMPLE_RATE / torch.clip(inputs[1], oracle.FMIN, oracle.FMAX)
    x = torch.cat((x, period[:, None]), dim=1)
    g = oracle.prepare_global_features(
        *inputs[4:7], state['speaker_embedding.weight'])
    return x, g.squeeze(2)
