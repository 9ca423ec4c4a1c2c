"""CPU restatement of HiFi-GAN streaming by overlap-save: the
schedule, stated in absolute frame ranges, driving any forward on windows of
the utterance - oracle/restatement.py's `hifigan_forward` in the CPU tests -
and the state with which the context is tight. Knows nothing of
promonet_amd: the tests compare the package's schedule and context with it.
"""
import torch

import restatement as oracle

# what `stream(defect=...)` can get wrong on purpose
DEFECTS = ('context', 'emit_offset', 'history_front', 'no_finish')


def ranges(chunks, left, lookahead, defect=None):
    """The steps of a stream fed `chunks` frames at a time, then finished:
    [(window_first, window_last, emit_first, emit_last, previous window)],
    absolute frames, `last` exclusive. After frames [0, p) audio is out for
    [0, max(0, p - lookahead)); a push of c frames emits up to
    max(0, p + c - lookahead) and synthesises the window that starts `left`
    frames before the first emitted frame (or at 0) and ends at p + c; the
    final step emits up to p on the window that ends at p.

    The window of a step is the tail of the previous window, then the chunk:
    `previous` is that window's (first, last), which `history_front` needs."""
    if defect == 'context':
        left -= 1
    steps, seen, previous = [], 0, (0, 0)
    for chunk in list(chunks) + [None]:
        final = chunk is None
        if final and defect == 'no_finish':
            break
        end = seen if final else seen + chunk
        first = max(0, seen - lookahead)
        last = end if final else max(0, end - lookahead)
        start = max(0, first - left)
        steps.append((start, end, first, last, previous))
        previous, seen = (start, end), end
    return steps


def stream(chunks, left, lookahead, forward, hop, defect=None):
    """The audio of every step, a list of (B, 1, hop * emitted) tensors (the
    last one is `finish`'s). `forward(first, last)` synthesises frames
    [first, last) of the utterance as an utterance of their own and returns
    (B, 1, hop * (last - first)); a window whose history is wrong is passed
    as a list of ranges to concatenate."""
    audio = []
    for start, end, first, last, previous in ranges(
            chunks, left, lookahead, defect):
        if last == first:
            audio.append(None)
            continue
        window = (start, end)
        if defect == 'history_front' and previous[0] < start:
            # the history taken from the front of the previous window
            keep = previous[1] - start
            window = [(previous[0], previous[0] + keep), (previous[1], end)]
        out = forward(*window) if isinstance(window, tuple) else forward(window)
        offset = first - start + (defect == 'emit_offset')
        audio.append(out[..., offset * hop:(offset + last - first) * hop])
    shape = next(a for a in audio if a is not None)
    return [shape[..., :0] if a is None else a for a in audio]


def same(streamed, full):
    """The comparison of the streaming tests: the concatenated audio of the
    steps has the full forward's shape and its bits"""
    joined = torch.cat(list(streamed), dim=-1)
    return joined.shape == full.shape and torch.equal(joined, full)


def close(streamed, full, tolerance):
    """`same` up to `tolerance` (float64 on the CPU: rounding)"""
    joined = torch.cat(list(streamed), dim=-1)
    return joined.shape == full.shape and \
        (joined - full).abs().max().item() <= tolerance


###############################################################################
# The state with which every frame of the context matters
###############################################################################


def outer_tap_state(rates, kernels, res_kernels, res_dilations,
                    initial_channels=16, features=4):
    """float64 weights for `restatement.hifigan_forward` (folded keys): every
    Conv1d has its two outermost taps only, 1 / (2 C_in) each, every
    transposed conv all its taps; no bias, no speaker conditioning. With
    positive inputs everything stays positive (LeakyReLU is the identity), so
    a contribution that is missing cannot cancel: the receptive field is
    exactly the interval arithmetic's."""
    def conv(cout, cin, k):
        w = torch.zeros(cout, cin, k, dtype=torch.float64)
        w[..., 0] = w[..., -1] = 1. / (2 * cin)
        return w

    c0 = initial_channels
    state = {
        'model.input_feature_conv.weight': conv(c0, features, 7),
        'model.input_feature_conv.bias': torch.zeros(c0, dtype=torch.float64),
        'model.input_speaker_conv.weight':
            torch.zeros(c0, 1, 1, dtype=torch.float64),
        'model.input_speaker_conv.bias': torch.zeros(c0, dtype=torch.float64)}
    for i, (r, k) in enumerate(zip(rates, kernels)):
        cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
        state[f'model.model.{i}.model.1.weight'] = torch.full(
            (cin, cout, k), float(r) / (cin * k), dtype=torch.float64)
        state[f'model.model.{i}.model.1.bias'] = torch.zeros(
            cout, dtype=torch.float64)
        for j, ks in enumerate(res_kernels):
            for name in ('convs1', 'convs2'):
                for n in range(len(res_dilations[j])):
                    prefix = f'model.model.{i}.model.2.model.{j}.{name}.{n}'
                    state[prefix + '.weight'] = conv(cout, cout, ks)
                    state[prefix + '.bias'] = torch.zeros(
                        cout, dtype=torch.float64)
    n = len(rates)
    state[f'model.model.{n + 1}.weight'] = conv(1, c0 // 2 ** n, 7)
    return state


def positive_inputs(batch, channels, frames, seed=0):
    """Features in [1e-6, 2e-6]: LeakyReLU and tanh stay linear"""
    gen = torch.Generator().manual_seed(seed)
    return 1e-6 * (1. + torch.rand(
        batch, channels, frames, generator=gen, dtype=torch.float64))


def window_forward(features, state):
    """`forward(first, last)` for `stream`: hifigan_forward of frames
    [first, last) (or of a list of such ranges, concatenated), every window
    computed once"""
    done = {}
    zero = torch.zeros(1, 1, 1, dtype=features.dtype)

    def forward(first, last=None):
        key = (first, last) if last is not None else tuple(first)
        if key not in done:
            pieces = [(first, last)] if last is not None else first
            window = torch.cat([features[..., a:b] for a, b in pieces], dim=-1)
            with torch.inference_mode():
                done[key] = oracle.hifigan_forward(window, zero, state)
        return done[key]
    return forward
