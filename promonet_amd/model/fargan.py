"""FARGAN vocoder running on the MI355X HIP engine.

Drop-in for `promonet.model.FARGAN` (promonet/model/fargan.py:13-131,
selected by `config/fargan.py`): same constructor arguments, same
`forward(features, global_features, previous_samples)` and
`step(features, global_features, previous_samples, states)`, same
`state_dict()` keys (weight-normed Linear layers keep `weight_g` /
`weight_v`). The whole frame-autoregressive loop - 4 sub-frame steps per
frame, the pitch lookback gather, three GRU cells, GLUs - runs inside one
persistent kernel per utterance (`pm_fargan_forward`, or
`pm_fargan_forward_stateful` from a carried recurrent state); there is no
PyTorch compute path.
"""
import math

import torch

import promonet_amd
from promonet_amd import _lib
from .core import attach
from .engine import EngineModule, device_lengths, global_features

# the recurrent state (fargan.py:406-415): three GRU states and the last
# sub-frame's input [features 128 | previous subframe 64 | lookback 68]
STATE_SIZES = (256, 256, 256, 260)


def initialize_recurrent_state(batch_size, device):
    """Zero recurrent state with the reference's shapes (fargan.py:406-415):
    (B, 256) x 3 and (B, 260), fp32."""
    return tuple(
        torch.zeros(batch_size, size, dtype=torch.float32, device=device)
        for size in STATE_SIZES)


class FARGAN(EngineModule):

    ABI = 'fargan'

    # auto mode: calls served by the one-workgroup-per-utterance kernel after
    # the cluster exchange has timed out twice in a row, before the clusters
    # are tried again
    RETRY_AFTER = 16

    def __init__(self, num_features, global_channels):
        super().__init__()
        self.num_features = num_features
        self.global_channels = global_channels
        self.hopsize = promonet_amd.HOPSIZE
        self.weight_dtype = promonet_amd.FARGAN_WEIGHT_DTYPE
        self.check_exchange = True
        self.kernel_mode = 0    # 0 auto, 1 workgroup per utterance, 2 clusters
        self._fallback_calls = 0    # auto mode: calls left on the slow kernel
        for key, tensor in self._initial_state().items():
            attach(self, key, tensor)

    def _initial_state(self):
        """Reference init: orthogonal Linear weights (fargan.py:418-424),
        GRUCell default U(-1/sqrt(H), 1/sqrt(H)), weight-norm g = ||v||."""
        hop, sub = self.hopsize, self.hopsize // 4
        channels = self.num_features + self.global_channels
        state = {}

        def orthogonal(rows, cols):
            return torch.nn.init.orthogonal_(torch.empty(rows, cols))

        def normed(prefix, rows, cols):
            v = orthogonal(rows, cols)
            state[prefix + '.weight_g'] = torch.linalg.vector_norm(
                v, dim=1, keepdim=True)
            state[prefix + '.weight_v'] = v

        state['conditioning_network.0.weight'] = orthogonal(channels, channels)
        state['conditioning_network.2.weight'] = orthogonal(channels, channels)
        state['conditioning_network.4.weight'] = orthogonal(2 * hop, channels)
        p = 'subframe_network.'
        normed(p + 'framewise_convolution.model.0', hop, 2 * (4 * sub + 4))
        normed(p + 'framewise_convolution.model.2.gate', hop, hop)
        bound = 1. / math.sqrt(hop)
        for n in (1, 2, 3):
            state[p + f'gru{n}.weight_ih'] = torch.empty(
                3 * hop, hop + 2 * sub).uniform_(-bound, bound)
            state[p + f'gru{n}.weight_hh'] = torch.empty(
                3 * hop, hop).uniform_(-bound, bound)
        for name in ('gru1_glu', 'gru2_glu', 'gru3_glu', 'skip_glu'):
            normed(p + name + '.gate', hop, hop)
        state[p + 'skip_dense.weight'] = orthogonal(hop, 4 * hop + 2 * sub)
        state[p + 'output_layer.weight'] = orthogonal(sub, hop)
        return state

    ###########################################################################
    # Engine (handle lifetime, workspace and stream guard: engine.py)
    ###########################################################################

    def _key(self):
        return self.weight_dtype

    def _create(self, lib, handle):
        return lib.pm_fargan_create(
            self.num_features, self.global_channels,
            _lib.DTYPES[self.weight_dtype], handle)

    ###########################################################################
    # Forward (fargan.py:21-59)
    ###########################################################################

    def forward(self, features, global_features, previous_samples):
        """features (B, 114, T) with the pitch period in samples as the last
        channel, global_features (B|1, 258, 1), previous_samples
        (B|1, 1, 512) -> (B, 1, 256 T). Unlike the reference (whose gather
        needs previous_samples expanded to the batch, fargan.py:238-241),
        batch-1 globals / previous samples broadcast."""
        return self._run(features, global_features, previous_samples, False)

    def forward_channels_last(
        self, features_cl, global_features, previous_samples, lengths=None
    ):
        """`lengths` (B,) frames: ragged batch of zero-padded utterances, each
        synthesised exactly as if alone (the model is causal); tails are 0."""
        return self._run(
            features_cl, global_features, previous_samples, True, lengths)

    ###########################################################################
    # Streaming (fargan.py:65-131)
    ###########################################################################

    def step(self, features, global_features, previous_samples, states):
        """Generate one frame from a recurrent state, as the reference's
        `FARGAN.step`: features (B, 114) with the pitch period last,
        global_features (B|1, 258[, 1]), previous_samples (B|1, 1, 512),
        states the 4-tuple of `initialize_recurrent_state` ->
        (signal (B, 256), previous_samples (B, 1, 512), states)."""
        if features.ndim != 2:
            raise ValueError('step: features must be (B, 114)')
        signal, previous_samples, states = self.stream(
            features[:, :, None], global_features, previous_samples, states)
        return signal[:, 0], previous_samples, states

    def stream(
        self, features, global_features, previous_samples=None, states=None,
        channels_last=False
    ):
        """Synthesise a chunk of frames from a recurrent state and return the
        state after it: features (B, 114, T) (or channels-last (B, T, 128)),
        previous_samples (B|1, 1, 512) or None, states a 4-tuple or None
        (zeros) -> (signal (B, 1, 256 T), previous_samples (B, 1, 512),
        states). Consecutive chunks carrying the state equal `forward` over
        the concatenated frames bit for bit."""
        batch = features.shape[0]
        if states is not None:
            states = tuple(states)
            if len(states) != len(STATE_SIZES) or any(
                    tuple(t.shape) != (batch, size)
                    for t, size in zip(states, STATE_SIZES)):
                raise ValueError(
                    'states must be (B, 256) x 3 and (B, 260) with the '
                    "features' batch")
            for tensor in states:
                _lib.require_gpu(tensor)
            states = torch.cat(states, dim=1).to(torch.float32).contiguous()
        signal, previous, states = self._run(
            features, global_features, previous_samples, channels_last,
            states=states, stateful=True)
        return (signal, previous[:, None],
                tuple(states.split(STATE_SIZES, dim=1)))

    def _run(self, x, g, previous, channels_last, lengths=None, states=None,
             stateful=False):
        _lib.require_gpu(x)
        engine = self.engine()
        lib = _lib.lib()
        x = x.to(torch.float32).contiguous()
        batch = x.shape[0]
        frames = x.shape[1] if channels_last else x.shape[2]
        if not channels_last and x.shape[1] != self.num_features + 1:
            raise ValueError(
                f'expected {self.num_features + 1} feature channels (the last '
                f'one is the pitch period), got {x.shape[1]}')
        g = global_features(g, batch, self.global_channels, x.device)
        pointer, pbatch = None, 1
        if previous is not None:
            previous = previous.reshape(previous.shape[0], -1).to(
                device=x.device, dtype=torch.float32).contiguous()
            if previous.shape[1] != 2 * self.hopsize or \
                    previous.shape[0] not in (1, batch):
                raise ValueError('previous_samples must be (B|1, 1, 512)')
            pointer, pbatch = _lib.ptr(previous), previous.shape[0]
        out = torch.empty(
            batch, 1, frames * self.hopsize, dtype=torch.float32,
            device=x.device)
        if stateful:
            if states is not None and states.device != x.device:
                raise ValueError('states must be on the features\' device')
            previous_out = torch.empty(
                batch, 2 * self.hopsize, dtype=torch.float32, device=x.device)
            states_out = torch.empty(
                batch, sum(STATE_SIZES), dtype=torch.float32, device=x.device)
        if lengths is not None:
            lengths = device_lengths(lengths, batch, x.device)
        if self.kernel_mode == 0 and not self.check_exchange:
            # the clusters' bounded waits are the only safety net of auto
            # mode: without the check a timed-out exchange would pass as
            # audio
            raise RuntimeError(
                'FARGAN: check_exchange=False needs an explicit '
                'kernel_mode (1 or 2)')
        if stateful:
            forward = 'pm_fargan_forward_stateful'
            tail = (_lib.ptr(states), _lib.ptr(out), _lib.ptr(previous_out),
                    _lib.ptr(states_out))
        elif lengths is None:
            forward, tail = 'pm_fargan_forward', (_lib.ptr(out),)
        else:
            forward = 'pm_fargan_forward_ragged'
            tail = (_lib.ptr(lengths, torch.int32), _lib.ptr(out))
        # (one claim of the workspace over every launch of the retry sequence)
        with self._claimed_workspace(
                engine, batch, frames, x.device) as workspace:

            def launch(mode):
                _lib.check(lib.pm_fargan_set_mode(engine, mode))
                _lib.check(getattr(lib, forward)(
                    engine, _lib.ptr(x), int(channels_last), _lib.ptr(g),
                    g.shape[0], pointer, pbatch, *tail, batch, frames,
                    workspace.data_ptr(), workspace.numel(), _lib.stream()))
                if self.check_exchange:
                    # the cluster kernel's inter-workgroup waits are bounded;
                    # a tripped bound must not pass as audio (one stream sync)
                    _lib.check(lib.pm_fargan_check(
                        engine, batch, frames, workspace.data_ptr(),
                        _lib.stream()))
            if self.kernel_mode == 0 and self._fallback_calls > 0:
                # the mode is chosen BEFORE the counter moves (the call that
                # takes it to 0 still runs the fallback kernel; the next one
                # tries the clusters again inside the guarded block below)
                launch(1)
                self._fallback_calls -= 1
                return (out, previous_out, states_out) if stateful else out
            try:
                launch(self.kernel_mode)
            except _lib.LibraryError as error:
                # The cluster kernel needs all its workgroups resident at
                # once; a GPU shared with another process (or CU-masked) can
                # break that and the bounded exchange gives up (PM_ETIMEOUT,
                # the audio of that launch is invalid). Auto mode retries the
                # clusters once - co-tenancy is often transient - and only
                # then runs this call on the one-workgroup-per-utterance
                # kernel; the clusters are tried again after RETRY_AFTER calls.
                if self.kernel_mode != 0 or error.code != _lib.PM_ETIMEOUT:
                    raise
                try:
                    launch(0)
                except _lib.LibraryError as again:
                    if again.code != _lib.PM_ETIMEOUT:
                        raise
                    import warnings
                    warnings.warn(
                        'FARGAN cluster exchange timed out twice (GPU shared '
                        'or partially masked?); using the one-workgroup-per-'
                        f'utterance kernel for the next {self.RETRY_AFTER} '
                        'calls')
                    self._fallback_calls = self.RETRY_AFTER
                    launch(1)
        return (out, previous_out, states_out) if stateful else out

    def remove_weight_norm(self):
        """No-op: weight norm is folded once at load."""
