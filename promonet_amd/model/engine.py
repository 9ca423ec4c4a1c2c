"""What every vocoder that wraps one C engine shares on the host.

`EngineModule` owns the engine handle (built lazily from `state_dict()`,
dropped whenever the parameters change), the grow-only workspace the engine
runs in, and the guard that keeps two streams out of that one workspace. A
subclass names its C symbols (`ABI`: `pm_{ABI}_load_tensor` / `finalize` /
`destroy` / `workspace_bytes`) and keeps what is its own: the part of the
engine key beside the device (`_key`) and the create call (`_create`).

Library functions are looked up through `_lib.lib()` at every call and never
kept: tests swap `_lib.lib` for a shim.
"""
import contextlib
import ctypes
import types

import torch

from promonet_amd import _lib


def global_features(g, batch, channels, device):
    """(B|1, G[, 1]) global features -> contiguous fp32 (B|1, G) on `device`"""
    g = g.reshape(g.shape[0], -1).to(
        device=device, dtype=torch.float32).contiguous()
    if g.shape[1] != channels or g.shape[0] not in (1, batch):
        raise ValueError(
            f'global features must be (B|1, {channels}[, 1]) with B = '
            f'{batch}, got {tuple(g.shape)}')
    return g


def device_lengths(lengths, batch, device):
    """`lengths` of a ragged batch -> contiguous int32 (B,) on `device`"""
    lengths = torch.as_tensor(lengths)
    if lengths.shape != (batch,):
        raise ValueError('lengths must have shape (B,)')
    return lengths.to(device=device, dtype=torch.int32).contiguous()


class EngineModule(torch.nn.Module):

    ABI = None      # 'hifigan' | 'fargan' | 'vocos'

    def __init__(self):
        super().__init__()
        self._engine = None
        self._engine_key = None
        self._generation = 0     # bumped whenever a live engine is dropped
        self._workspace = None
        self._busy = None        # (stream, event) of the last engine call
        self.register_load_state_dict_post_hook(
            lambda module, keys: module._invalidate())

    def _symbol(self, name):
        return getattr(_lib.lib(), f'pm_{self.ABI}_{name}')

    ###########################################################################
    # Engine lifetime
    ###########################################################################

    def _key(self):
        """What the packed engine depends on beside the device"""
        raise NotImplementedError

    def _create(self, lib, handle):
        """Call pm_{ABI}_create into `handle`; returns its status"""
        raise NotImplementedError

    def _invalidate(self):
        self._destroy()

    def _destroy(self):
        if getattr(self, '_engine', None) is not None:
            self._symbol('destroy')(self._engine)
            # (captured graphs hold the old engine's weight pointers:
            # Generator.packed_inference(graph=True) keys its cache on this)
            self._generation = getattr(self, '_generation', 0) + 1
        self._engine = None
        self._engine_key = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .half() move the parameters: repack lazily
        result = super()._apply(fn, *args, **kwargs)
        self._invalidate()
        return result

    def engine(self):
        """Create the HIP engine and (re)load every tensor when needed."""
        first = next(self.parameters())
        if not first.is_cuda:
            raise RuntimeError(
                f'promonet_amd.model.{type(self).__name__} runs on an AMD GPU '
                'only; move the model with .to("cuda:N") (no CPU fallback)')
        key = (first.device, self._key())
        if self._engine is not None and self._engine_key == key:
            return self._engine
        self._destroy()
        lib = _lib.lib()
        handle = ctypes.c_void_p()
        with torch.cuda.device(first.device):
            _lib.check(self._create(lib, ctypes.byref(handle)))
            try:
                for name, tensor in self.state_dict().items():
                    tensor = tensor.detach().to(torch.float32).contiguous()
                    _lib.check(self._symbol('load_tensor')(
                        handle, name.encode(), _lib.ptr(tensor),
                        _lib.shape_array(tensor.shape), tensor.ndim,
                        _lib.stream()))
                _lib.check(self._symbol('finalize')(handle, _lib.stream()))
            except Exception:
                self._symbol('destroy')(handle)
                raise
        self._engine = handle
        self._engine_key = key
        return handle

    ###########################################################################
    # Workspace
    ###########################################################################

    def _claim_workspace(self, device):
        """One workspace per module: a forward on stream B while the previous
        one is still running on stream A would overwrite the activations under
        it. Raise instead (same-stream calls are ordered by the stream; a
        different stream is fine once the previous forward has finished)."""
        stream = torch.cuda.current_stream(device)
        if torch.cuda.is_current_stream_capturing():
            return None
        if self._busy is not None:
            previous, event = self._busy
            if previous != stream and not event.query():
                raise RuntimeError(
                    f'promonet_amd.model.{type(self).__name__}: forward on '
                    f'{stream} while the previous forward is still running on '
                    f'{previous} - the module owns ONE workspace; wait for it '
                    '(stream.wait_stream / synchronize) or use one model per '
                    'stream')
            event = event if previous.device == stream.device \
                else torch.cuda.Event()
        else:
            event = torch.cuda.Event()
        return stream, event

    def _release_workspace(self, claim):
        if claim is not None:
            claim[1].record(claim[0])
            self._busy = claim

    @contextlib.contextmanager
    def _claimed_workspace(self, engine, batch, frames, device,
                           workspace_bytes=None):
        """The workspace of a (batch, frames) call, claimed for the current
        stream of `device` (made the current device) until the block ends;
        one claim may cover several launches. `workspace_bytes` names the
        sizing function where it is not pm_{ABI}_workspace_bytes."""
        with torch.cuda.device(device):
            claim = self._claim_workspace(device)
            try:
                size = getattr(
                    _lib.lib(),
                    workspace_bytes or f'pm_{self.ABI}_workspace_bytes')(
                        engine, batch, frames)
                if (
                    self._workspace is None or
                    self._workspace.numel() < size or
                    self._workspace.device != device
                ):
                    self._workspace = None      # released before the larger one
                    self._workspace = torch.empty(
                        size, dtype=torch.uint8, device=device)
                yield self._workspace
            finally:
                self._release_workspace(claim)

    def _call(self, name, engine, *leading, batch, frames, device,
              workspace_bytes=None):
        """`name`(engine, *leading, batch, frames, workspace, bytes, stream)
        inside a claim of the workspace"""
        with self._claimed_workspace(
                engine, batch, frames, device, workspace_bytes) as workspace:
            _lib.check(getattr(_lib.lib(), name)(
                engine, *leading, batch, frames, workspace.data_ptr(),
                workspace.numel(), _lib.stream()))

    @contextlib.contextmanager
    def private_workspace(self):
        """Calls inside the block run in a fresh workspace instead of the
        shared one - a captured graph's: the shared workspace may be
        re-allocated by a later, larger call, and a captured kernel keeps the
        pointer it was recorded with. Yields a holder whose `.tensor` is that
        workspace once the block has ended, for the caller to keep alive; the
        shared workspace is back then."""
        holder = types.SimpleNamespace(tensor=None)
        shared, self._workspace = self._workspace, None
        try:
            yield holder
        finally:
            holder.tensor, self._workspace = self._workspace, shared
