"""HiFi-GAN vocoder running on the MI355X HIP engine.

Drop-in for `promonet.model.HiFiGAN` (promonet/model/hifigan.py:13-77):
same constructor arguments, same `forward(x, g, p)` signature, same
`state_dict()` keys / shapes (weight-normed layers keep `weight_g` and
`weight_v`), so a reference `generator-*.pt` loads unchanged. The forward
pass is one call into `libpromonet_hip.so` (`pm_hifigan_forward`); there is
no PyTorch compute path and no CPU fallback.
"""
import ctypes
import math

import torch

import promonet_amd
from promonet_amd import _lib
from .core import attach
from .engine import EngineModule, device_lengths, global_features


def checkpoint_schedule(stages):
    """The operand types 'checkpoint' (config.py) stands for, one per upsampling
    stage: f16 everywhere; in the LAST stage the activations split into hi + lo
    ('f16a2': its Blocks two MFMAs per step, its upsampler fully split), and
    the upsampler in front of the second-to-last stage fully split as well
    ('f16ux'). scripts/checkpoint_schedule.py measures the candidates."""
    if stages == 1:
        return ['f16a2']
    return ['f16'] * (stages - 2) + ['f16ux', 'f16a2']



def hifigan_context(rates, kernels, res_kernels, res_dilations):
    """(left, right): the frames before and after a frame that its audio
    depends on - the receptive field of the generator, by interval arithmetic
    backwards from the samples [0, hop) of frame 0 to the input frames they
    read (mirror of `pm_hifigan_context`). (13, 13) at the
    defaults."""
    first, last = 0, math.prod(rates) - 1
    first, last = first - 3, last + 3                # output conv, k 7
    # the widest Block: per dilation d a conv (k, d) and a conv (k, 1)
    block = max(
        sum((k - 1) // 2 * d + (k - 1) // 2 for d in dilations)
        for k, dilations in zip(res_kernels, res_dilations))
    for r, k in reversed(list(zip(rates, kernels))):
        if k < r or (k - r) % 2:
            raise ValueError(
                f'upsampler rate {r} kernel {k}: the padding (k - r) / 2 must '
                'be a whole number')
        first, last = first - block, last + block
        # ConvTranspose1d(stride r, kernel k, padding q): out[n] reads x[m]
        # with 0 <= n + q - m r <= k - 1
        q = (k - r) // 2
        first, last = -((k - 1 - q - first) // r), (last + q) // r
    first, last = first - 3, last + 3                # input conv, k 7
    return -first, last


def stream_schedule(seen, chunk, left, lookahead, final=False):
    """One step of the overlap-save schedule: frames [0, seen)
    have been pushed, `chunk` more arrive (`final`: none do, the utterance
    ends at `seen`). Returns (keep, emit_first, emit_frames, seen after).

    The window of the step is [the last `keep` pushed frames | chunk]; the
    audio of its frames [emit_first, emit_first + emit_frames) is emitted.
    With lookahead R, audio is out for frames [0, max(0, seen - R)); the step
    emits up to max(0, seen + chunk - R) (up to `seen` when final), and the
    window starts `left` frames before the first emitted one - or at frame 0,
    where the zero padding of the convolutions is the truth."""
    if seen < 0 or chunk < 0 or left < 0 or lookahead < 0:
        raise ValueError('negative frame count')
    if final and chunk:
        raise ValueError('the final step takes no frames')
    keep = min(left + lookahead, seen)
    first = max(0, seen - lookahead)
    last = seen if final else max(0, seen + chunk - lookahead)
    return keep, first - (seen - keep), last - first, seen + chunk


class HiFiGAN(EngineModule):

    ABI = 'hifigan'

    def __init__(self, initial_channel, gin_channels):
        super().__init__()
        self.initial_channel = initial_channel
        self.gin_channels = gin_channels
        self.channels = promonet_amd.HIFIGAN_UPSAMPLE_INITIAL_SIZE
        self.rates = list(promonet_amd.HIFIGAN_UPSAMPLE_RATES)
        self.kernels = list(promonet_amd.HIFIGAN_UPSAMPLE_KERNEL_SIZES)
        self.res_kernels = list(promonet_amd.HIFIGAN_RESBLOCK_KERNEL_SIZES)
        self.res_dilations = [
            list(d) for d in promonet_amd.HIFIGAN_RESBLOCK_DILATION_SIZES]
        self.compute_dtype = promonet_amd.COMPUTE_DTYPE
        self.hopsize = math.prod(self.rates)

        for key, tensor in self._initial_state().items():
            attach(self, key, tensor)

    ###########################################################################
    # Parameters (reference init: hifigan.py:19-61, 220-223)
    ###########################################################################

    def _initial_state(self):
        state = {}

        def default_conv(prefix, cout, cin, k, bias=True):
            # torch.nn.Conv1d default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
            bound = 1. / math.sqrt(cin * k)
            state[f'{prefix}.weight'] = torch.empty(
                cout, cin, k).uniform_(-bound, bound)
            if bias:
                state[f'{prefix}.bias'] = torch.empty(
                    cout).uniform_(-bound, bound)

        def weight_normed(prefix, shape, nbias, fan_in):
            v = torch.randn(*shape) * .01
            bound = 1. / math.sqrt(fan_in)
            state[f'{prefix}.bias'] = torch.empty(nbias).uniform_(-bound, bound)
            state[f'{prefix}.weight_g'] = torch.linalg.vector_norm(
                v, dim=(1, 2), keepdim=True)
            state[f'{prefix}.weight_v'] = v

        c0 = self.channels
        default_conv('input_feature_conv', c0, self.initial_channel, 7)
        default_conv('input_speaker_conv', c0, self.gin_channels, 1)
        for i, (r, k) in enumerate(zip(self.rates, self.kernels)):
            cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
            weight_normed(
                f'model.{i}.model.1', (cin, cout, k), cout, cout * k)
            for j, ks in enumerate(self.res_kernels):
                for name in ('convs1', 'convs2'):
                    for n in range(len(self.res_dilations[j])):
                        weight_normed(
                            f'model.{i}.model.2.model.{j}.{name}.{n}',
                            (cout, cout, ks), cout, cout * ks)
        n = len(self.rates)
        default_conv(f'model.{n + 1}', 1, c0 // 2 ** n, 7, bias=False)
        return state

    ###########################################################################
    # Engine (handle lifetime, workspace and stream guard: engine.py)
    ###########################################################################

    def _key(self):
        return self.compute_dtype

    def _create(self, lib, handle):
        config = _lib.HifiganConfig()
        config.num_features = self.initial_channel
        config.global_channels = self.gin_channels
        config.initial_channels = self.channels
        config.num_stages = len(self.rates)
        for i, (r, k) in enumerate(zip(self.rates, self.kernels)):
            config.upsample_rates[i] = r
            config.upsample_kernel_sizes[i] = k
        config.num_resblocks = len(self.res_kernels)
        config.num_dilations = len(self.res_dilations[0])
        for j, k in enumerate(self.res_kernels):
            config.resblock_kernel_sizes[j] = k
            if len(self.res_dilations[j]) != config.num_dilations:
                raise ValueError('ragged dilation lists are not supported')
            for n, d in enumerate(self.res_dilations[j]):
                config.resblock_dilations[j][n] = d
        # 'checkpoint' / 'bf16' / 'f16' / 'fp32' / 'f16x3', or one operand type
        # per upsampling stage joined by '+' ('bf16+bf16+f16+f16': the input
        # conv takes the first)
        per_stage = str(self.compute_dtype).split('+')
        if per_stage == ['checkpoint']:
            per_stage = checkpoint_schedule(len(self.rates))
        if len(per_stage) not in (1, len(self.rates)):
            raise ValueError(
                f'COMPUTE_DTYPE {self.compute_dtype!r}: one operand type, or '
                f'one per stage ({len(self.rates)})')
        config.compute_dtype = _lib.DTYPES[per_stage[0]]
        if len(per_stage) > 1:
            for i, name in enumerate(per_stage):
                config.stage_compute_dtype[i] = 1 + _lib.DTYPES[name]
        return lib.pm_hifigan_create(ctypes.byref(config), handle)

    ###########################################################################
    # Forward
    ###########################################################################

    def forward(self, x, g, p=None):
        """x (B, C, T) features, g (B|1, G, 1) globals -> (B, 1, T * hop).

        `p` (previous samples) is accepted and ignored, as in the reference
        (promonet/model/hifigan.py:63)."""
        return self._run(x, g, channels_last=False)

    def forward_channels_last(self, x_cl, g, lengths=None):
        """x_cl (B, T, C_pad) as written by `pm_prepare_features`; `lengths`
        (B,) frames makes the batch ragged: every utterance is synthesised
        as if alone, the audio past its end is zero."""
        return self._run(x_cl, g, channels_last=True, lengths=lengths)

    def _run(self, x, g, channels_last, lengths=None):
        _lib.require_gpu(x)
        engine = self.engine()
        x = x.to(torch.float32).contiguous()
        batch = x.shape[0]
        frames = x.shape[1] if channels_last else x.shape[2]
        g = global_features(g, batch, self.gin_channels, x.device)
        if not channels_last and x.shape[1] != self.initial_channel:
            raise ValueError(
                f'expected {self.initial_channel} feature channels, '
                f'got {x.shape[1]}')
        out = torch.empty(
            batch, 1, frames * self.hopsize, dtype=torch.float32,
            device=x.device)
        if lengths is not None:
            lengths = device_lengths(lengths, batch, x.device)
            self._call(
                'pm_hifigan_forward_ragged', engine, _lib.ptr(x),
                int(channels_last), _lib.ptr(g), g.shape[0],
                _lib.ptr(lengths, torch.int32), _lib.ptr(out), batch=batch,
                frames=frames, device=x.device)
        else:
            self._call(
                'pm_hifigan_forward_cl' if channels_last
                else 'pm_hifigan_forward', engine, _lib.ptr(x), _lib.ptr(g),
                g.shape[0], _lib.ptr(out), batch=batch, frames=frames,
                device=x.device)
        return out

    ###########################################################################
    # Streaming
    ###########################################################################

    def context(self):
        """(left, right) frames of context a frame's audio depends on"""
        return hifigan_context(
            self.rates, self.kernels, self.res_kernels, self.res_dilations)

    def open_stream(self, global_features, batch, lookahead=None, graph=False):
        """A `HiFiGANStream` of `batch` rows in lockstep: chunks of frames in,
        audio out, the concatenated audio bit for bit one `forward` over the
        concatenated frames. `lookahead` frames are held back (None: the
        right context, exact; fewer: every push emits what `forward` gives
        for an utterance that ends where the stream has got to); `graph`
        replays a captured hipGraph per window shape."""
        return HiFiGANStream(self, global_features, batch, lookahead, graph)

    def remove_weight_norm(self):
        """No-op: the engine folds weight norm once at load
        (reference: hifigan.py:72-77 only matters for TorchScript export)."""


class HiFiGANStream:
    """Overlap-save streaming of one `HiFiGAN`. Every push
    synthesises a window - the last `keep` frames pushed before, then the
    chunk - with the engine's ordinary forward (`pm_hifigan_stream`) and
    emits the frames whose context the window holds. State: two window
    buffers the steps swap between, the count of frames seen, a workspace of
    the stream's own and, with `graph`, one captured graph per window shape
    and buffer phase."""

    # captured graphs kept per stream, oldest dropped first
    MAX_PACKED_GRAPHS = 8

    def __init__(self, model, global_features_, batch, lookahead=None,
                 graph=False):
        device = next(model.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError(
                'promonet_amd.model.HiFiGAN runs on an AMD GPU only; move the '
                'model with .to("cuda:N") (no CPU fallback)')
        self.model = model
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError('batch must be at least 1')
        self.left, self.right = model.context()
        self.lookahead = self.right if lookahead is None else int(lookahead)
        if not 0 <= self.lookahead <= self.right:
            raise ValueError(
                f'lookahead must lie in [0, {self.right}] (the right context '
                f'of the generator), got {lookahead}')
        self.graph = bool(graph)
        self.device = device
        self.channels = model.initial_channel
        self.channels_padded = (self.channels + 31) // 32 * 32
        # (outside inference mode: `set_global_features` writes in place)
        with torch.inference_mode(False):
            self.g = global_features(
                global_features_, self.batch, model.gin_channels,
                device).clone()
        self._graphs = {}        # captured steps, oldest first
        self._shapes = set()     # the (keep, chunk) shapes run eagerly once
        self._generation = model._generation
        self._workspace = None
        self.reset()

    def reset(self):
        """Back to the start of an utterance (captured graphs are kept)"""
        self.seen = 0
        self.closed = False
        self._windows = getattr(self, '_windows', [None, None])
        self._phase = 0          # the buffer that holds the current window
        self._frames = 0         # frames of the current window

    def set_global_features(self, global_features_):
        """Replace the global features, in place (a captured graph reads the
        same tensor)"""
        self.g.copy_(global_features(
            global_features_, self.g.shape[0], self.model.gin_channels,
            self.device))

    ###########################################################################
    # Steps
    ###########################################################################

    def push(self, features, channels_last=False, prepare=None):
        """features (B, C, c) (or channels-last (B, c, C_pad)) ->
        (B, 1, hop * emitted) float32; nothing is emitted while the stream
        holds fewer than `lookahead` frames. With `prepare`, `features` is a
        raw chunk (..., c) of the caller's and `prepare(features)` gives its
        channels-last features (and may `set_global_features`): in graph mode
        it is captured with the step."""
        if self.closed:
            raise ValueError('push after finish: reset() starts a new stream')
        _lib.require_gpu(features)
        if prepare is not None:
            features = features.to(torch.float32).contiguous()
            chunk = features.shape[-1]
            if chunk == 0:
                return self._empty()
            keep, first, count, seen = stream_schedule(
                self.seen, chunk, self.left, self.lookahead)
            audio = self._step(
                features, True, chunk, keep, first, count, prepare)
            self.seen = seen
            return audio
        expected = (
            (self.batch, None, self.channels_padded) if channels_last else
            (self.batch, self.channels, None))
        if features.ndim != 3 or any(
                want is not None and want != have
                for want, have in zip(expected, features.shape)):
            raise ValueError(
                f'expected features of shape {expected} (None: the frames of '
                f'the chunk), got {tuple(features.shape)}')
        features = features.to(torch.float32).contiguous()
        chunk = features.shape[1] if channels_last else features.shape[2]
        if chunk == 0:
            return self._empty()
        keep, first, count, seen = stream_schedule(
            self.seen, chunk, self.left, self.lookahead)
        audio = self._step(features, channels_last, chunk, keep, first, count)
        self.seen = seen
        return audio

    def finish(self):
        """The audio of the last `lookahead` frames: the utterance ends where
        the stream has got to. Closes the stream."""
        if self.closed:
            raise ValueError('finish after finish: reset() starts a new stream')
        keep, first, count, _ = stream_schedule(
            self.seen, 0, self.left, self.lookahead, final=True)
        self.closed = True
        if count == 0:
            return self._empty()
        return self._step(None, True, 0, keep, first, count)

    def _empty(self):
        return torch.empty(
            self.batch, 1, 0, dtype=torch.float32, device=self.device)

    def _window(self, index, frames):
        """Window buffer `index`, at least `frames` long"""
        window = self._windows[index]
        if window is None or window.shape[1] < frames:
            # (room for the steady state of this chunk size, so that a stream
            # of equal chunks allocates each buffer once)
            room = max(frames, self.left + self.lookahead + frames)
            window = self._windows[index] = torch.empty(
                self.batch, room, self.channels_padded, dtype=torch.float32,
                device=self.device)
        return window

    def _step(self, features, channels_last, chunk, keep, first, count,
              prepare=None):
        previous = self._windows[self._phase]
        window = self._window(1 - self._phase, keep + chunk)
        step = (chunk, int(channels_last), self._frames, keep, first, count)
        if self.graph and count and features is not None:
            audio = self._replay(features, previous, window, step, prepare)
        else:
            audio = self._launch(
                prepare(features) if prepare else features, previous, window,
                step)
        self._phase = 1 - self._phase
        self._frames = keep + chunk
        return audio

    def _launch(self, features, previous, window, step):
        """One `pm_hifigan_stream` call in the stream's own workspace"""
        chunk, channels_last, frames, keep, first, count = step
        model = self.model
        engine = model.engine()
        out = torch.empty(
            self.batch, 1, count * model.hopsize, dtype=torch.float32,
            device=self.device)
        with model.private_workspace() as private:
            model._workspace = self._workspace
            with model._claimed_workspace(
                    engine, self.batch, keep + chunk, self.device,
                    'pm_hifigan_stream_workspace_bytes') as workspace:
                _lib.check(_lib.lib().pm_hifigan_stream(
                    engine, _lib.ptr(features), channels_last, chunk,
                    _lib.ptr(previous) if keep else None, frames, keep,
                    _lib.ptr(window), _lib.ptr(self.g), self.g.shape[0],
                    first, count, _lib.ptr(out) if count else None,
                    self.batch, workspace.data_ptr(), workspace.numel(),
                    _lib.stream()))
        self._workspace = private.tensor
        return out

    ###########################################################################
    # Graph mode (as Generator._packed_graph)
    ###########################################################################

    def _replay(self, features, previous, window, step, prepare):
        """The first step of a (keep, chunk) shape runs eagerly (the engine
        packed, the kernels' host-side constants cached); from the second on
        it is captured - once per pair of buffers it swaps between - and
        replayed. A stream of equal chunks settles on two graphs."""
        self.model.engine()                    # (re)built outside any capture
        cache, shapes = self._graphs, self._shapes
        if self._generation != self.model._generation:
            # new weights: the old graphs hold the old engine's pointers
            cache.clear()
            shapes.clear()
            self._generation = self.model._generation
        shape = (tuple(features.shape), step[0], step[1], step[3])
        if shape not in shapes:
            shapes.add(shape)
            return self._launch(
                prepare(features) if prepare else features, previous, window,
                step)
        key = (tuple(features.shape), step,
               previous.data_ptr() if previous is not None else 0,
               window.data_ptr())
        entry = cache.get(key)
        if entry is None:
            while len(cache) >= self.MAX_PACKED_GRAPHS:
                del cache[next(iter(cache))]
            entry = cache[key] = self._capture(
                features, previous, window, step, prepare)
        entry['input'].copy_(features)
        entry['graph'].replay()
        return entry['output'].clone()

    def _capture(self, features, previous, window, step, prepare):
        """The step as a graph on a static input, in a workspace of the
        graph's own (the stream's may be re-allocated by a larger step, and a
        captured kernel keeps the pointer it was recorded with)."""
        # (inference mode OFF: see Generator._capture_packed)
        with torch.inference_mode(False), torch.no_grad(), \
                torch.cuda.device(self.device):
            static = torch.empty(
                features.shape, dtype=features.dtype, device=self.device)
            static.copy_(features)
            held, self._workspace = self._workspace, None
            try:
                graph = torch.cuda.CUDAGraph()
                torch.cuda.synchronize(self.device)
                with torch.cuda.graph(graph):
                    output = self._launch(
                        prepare(static) if prepare else static, previous,
                        window, step)
                torch.cuda.synchronize(self.device)
            finally:
                workspace, self._workspace = self._workspace, held
        # (the windows too: a buffer the stream has outgrown stays alive as
        # long as a graph that reads or writes it)
        return {'graph': graph, 'input': static, 'output': output,
                'workspace': workspace, 'windows': (previous, window)}
