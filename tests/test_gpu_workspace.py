"""An entry of the C ABI that is given exactly the workspace its sizing
function asks for writes nothing behind it.

Every other test allocates exactly `*_bytes` and never looks behind them, so a
layout whose launch places a buffer past what the sizing function counted
would corrupt a neighbouring allocation unseen. Here the workspace is the
first half of one allocation whose second half is a guard pattern: a slot
placed too far lands in the guard, inside the same allocation, and shows as a
failed assertion. The outputs have to equal, bit for bit, those of the same
call in a separate, roomy workspace, and one byte less than `*_bytes` is
refused with PM_ENOMEM before anything is launched.

Shapes: the smallest that reach every slot of each layout."""
import ctypes

import pytest
import torch

import promonet_amd
from promonet_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def guarded(size, device):
    return torch.full((2 * size,), GUARD, dtype=torch.uint8, device=device)


def check_entry(device, size, call, required=None, roomy=None):
    """call(workspace tensor, bytes) -> (status, output tensors), fresh
    outputs at every call. `required`: what the entry refuses to go under
    (`size` itself unless the tail of `size` is optional scratch; 0: the
    entry takes no size). `roomy`: the bytes the roomy run announces."""
    assert size > 0
    required = size if required is None else required
    reference = guarded(size, device)
    code, want = call(reference, 2 * size if roomy is None else roomy)
    assert code == 0, _lib.lib().pm_last_error()
    workspace = guarded(size, device)
    code, got = call(workspace, size)
    assert code == 0, _lib.lib().pm_last_error()
    torch.cuda.synchronize()
    assert bool((workspace[size:] == GUARD).all()), 'wrote behind *_bytes'
    assert len(got) == len(want) and len(got) > 0
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    if required:
        code, _ = call(workspace, required - 1)
        assert code == _lib.PM_ENOMEM
    return workspace


def randn(gen, device, *shape, scale=1.):
    return (torch.randn(*shape, generator=gen) * scale).to(device).contiguous()


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def conv_weights(gen, device, channels, kernel_size, count):
    std = 1. / (channels * kernel_size) ** .5
    return {
        'w1': [randn(gen, device, channels, channels, kernel_size, scale=std)
               for _ in range(count)],
        'b1': [randn(gen, device, channels, scale=.1) for _ in range(count)],
        'w2': [randn(gen, device, channels, channels, kernel_size, scale=std)
               for _ in range(count)],
        'b2': [randn(gen, device, channels, scale=.1) for _ in range(count)]}


def test_block_iteration(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(1)
    c, k, batch, length = 32, 3, 1, 64
    x = randn(gen, device, batch, length, c)
    t = conv_weights(gen, device, c, k, 1)

    def call(ws, nbytes):
        out = torch.zeros_like(x)
        return lib.pm_block_iteration_cl(
            _lib.PM_F16, _lib.ptr(x), _lib.ptr(out), _lib.ptr(t['w1'][0]),
            _lib.ptr(t['b1'][0]), _lib.ptr(t['w2'][0]), _lib.ptr(t['b2'][0]),
            batch, length, c, k, 1, 0, 1., ws.data_ptr(), nbytes,
            _lib.stream()), [out]
    check_entry(device, lib.pm_op_workspace_bytes(c, c, k), call)


def test_block_with_walk_scratch(device):
    """The skewed walk of the 4-byte operand layout, forced: the bytes behind
    the packed weights are its scratch. (The roomy run announces the same
    bytes: more scratch may plan another launch.)"""
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(2)
    c, k, batch, length = 32, 11, 2, 256
    x = randn(gen, device, batch, length, c)
    t = conv_weights(gen, device, c, k, 3)
    dilations = (ctypes.c_int * 3)(1, 3, 5)
    weights = 3 * lib.pm_op_workspace_bytes(c, c, k)
    size = weights + lib.pm_walk_scratch_bytes(batch)

    def call(ws, nbytes):
        out = torch.zeros_like(x)
        return lib.pm_block_cl(
            _lib.PM_F32, _lib.ptr(x), _lib.ptr(out), pointers(t['w1']),
            pointers(t['b1']), pointers(t['w2']), pointers(t['b2']),
            dilations, 3, batch, length, c, k, 0, 1., ws.data_ptr(), nbytes,
            _lib.stream()), [out]
    try:
        _lib.check(lib.pm_debug_force(2, 0))
        ws = check_entry(
            device, size, call, required=weights, roomy=size)
        used = int((ws[weights:size] != GUARD).sum())
        print(f'walk scratch: {used} of {size - weights} bytes written')
    finally:
        _lib.check(lib.pm_debug_force(0, 0))


def test_mrf(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(3)
    c, batch, length = 32, 2, 256
    x = randn(gen, device, batch, length, c)
    t = {name: [] for name in ('w1', 'b1', 'w2', 'b2')}
    for k in (3, 7, 11):
        for name, tensors in conv_weights(gen, device, c, k, 3).items():
            t[name] += tensors
    dilations = (ctypes.c_int * 3)(1, 3, 5)
    size = 9 * lib.pm_op_workspace_bytes(c, c, 11)

    def call(ws, nbytes):
        out = torch.zeros_like(x)
        return lib.pm_mrf_cl(
            _lib.PM_F16, _lib.ptr(x), _lib.ptr(out), pointers(t['w1']),
            pointers(t['b1']), pointers(t['w2']), pointers(t['b2']),
            dilations, 3, batch, length, c, ws.data_ptr(), nbytes,
            _lib.stream()), [out]
    # (the roomy run announces the same bytes: more would be walk scratch)
    check_entry(device, size, call, roomy=size)


def test_input_conv(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(4)
    c_in, c_out, channels, batch, length = 32, 64, 8, 2, 64
    x = randn(gen, device, batch, length, c_in)
    w = randn(gen, device, c_out, c_in, 7, scale=1. / (c_in * 7) ** .5)
    bias = randn(gen, device, c_out, scale=.1)
    g = randn(gen, device, batch, channels)
    speaker_w = randn(gen, device, c_out, channels, 1, scale=.3)
    speaker_b = randn(gen, device, c_out, scale=.1)
    size = lib.pm_op_workspace_bytes(c_in, c_out, 7) + \
        256 * ((batch * c_out * 4 + 255) // 256)

    def call(ws, nbytes):
        out = torch.zeros(batch, length, c_out, device=device)
        return lib.pm_input_conv_cl(
            _lib.PM_F16, _lib.ptr(x), _lib.ptr(out), _lib.ptr(w),
            _lib.ptr(bias), _lib.ptr(g), _lib.ptr(speaker_w),
            _lib.ptr(speaker_b), batch, channels, batch, length, c_in, c_out,
            ws.data_ptr(), nbytes, _lib.stream()), [out]
    check_entry(device, size, call)


def test_conv_transpose(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(5)
    c_in, c_out, rate, batch, length = 64, 32, 2, 1, 64
    x = randn(gen, device, batch, length, c_in)
    w = randn(gen, device, c_in, c_out, 2 * rate, scale=1. / (2 * c_in) ** .5)
    bias = randn(gen, device, c_out, scale=.1)

    def call(ws, nbytes):
        out = torch.zeros(batch, length * rate, c_out, device=device)
        return lib.pm_conv_transpose_cl(
            _lib.PM_F16, _lib.ptr(x), _lib.ptr(out), _lib.ptr(w),
            _lib.ptr(bias), batch, length, c_in, c_out, rate, 1,
            ws.data_ptr(), nbytes, _lib.stream()), [out]
    check_entry(
        device, lib.pm_op_workspace_bytes(c_in, c_out, 2 * rate), call)


# every tensor of a Vocos engine with `layers` ConvNeXt blocks
def vocos_shapes(layers, features=80, global_channels=256, c=512, h=1536):
    shapes = {
        'conv_pre.weight': (c, features, 7), 'conv_pre.bias': (c,),
        'cond.weight': (c, global_channels, 1), 'cond.bias': (c,),
        'backbone.embed.weight': (c, c, 7), 'backbone.embed.bias': (c,),
        'backbone.norm.weight': (c,), 'backbone.norm.bias': (c,),
        'backbone.final_layer_norm.weight': (c,),
        'backbone.final_layer_norm.bias': (c,),
        'head.out.weight': (1026, c), 'head.out.bias': (1026,),
        'head.istft.window': (1024,)}
    for i in range(layers):
        prefix = f'backbone.convnext.{i}.'
        shapes.update({
            prefix + 'dwconv.weight': (c, 1, 7), prefix + 'dwconv.bias': (c,),
            prefix + 'norm.weight': (c,), prefix + 'norm.bias': (c,),
            prefix + 'pwconv1.weight': (h, c), prefix + 'pwconv1.bias': (h,),
            prefix + 'pwconv2.weight': (c, h), prefix + 'pwconv2.bias': (c,),
            prefix + 'gamma': (c,)})
    return shapes


def vocos_state(gen, device, layers):
    state = {}
    for name, shape in vocos_shapes(layers).items():
        if name.endswith('window'):
            tensor = torch.hann_window(1024)
        elif 'norm.weight' in name:
            tensor = 1. + .1 * torch.randn(*shape, generator=gen)
        else:
            tensor = .05 * torch.randn(*shape, generator=gen)
        state[name] = tensor.to(device).contiguous()
    return state


def test_convnext_block(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(6)
    batch, frames, c, h = 1, 8, 512, 1536
    state = vocos_state(gen, device, 1)
    x = randn(gen, device, batch, frames, c)
    names = ('dwconv.weight', 'dwconv.bias', 'norm.weight', 'norm.bias',
             'pwconv1.weight', 'pwconv1.bias', 'pwconv2.weight',
             'pwconv2.bias', 'gamma')

    def call(ws, nbytes):
        y = torch.zeros_like(x)
        return lib.pm_convnext_block_cl(
            _lib.PM_F16, _lib.ptr(x), _lib.ptr(y),
            *[_lib.ptr(state['backbone.convnext.0.' + n]) for n in names],
            batch, frames, c, h, ws.data_ptr(), nbytes, _lib.stream()), [y]
    check_entry(
        device, lib.pm_convnext_block_workspace_bytes(_lib.PM_F16, c, h), call)


def test_vocos_head(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(7)
    batch, frames = 2, 4
    state = vocos_state(gen, device, 0)
    x = randn(gen, device, batch, frames, 512)

    def call(ws, nbytes):
        audio = torch.zeros(batch, frames * 256, device=device)
        return lib.pm_vocos_head(
            _lib.PM_F16, _lib.ptr(x), _lib.ptr(state['head.out.weight']),
            _lib.ptr(state['head.out.bias']),
            _lib.ptr(state['head.istft.window']), _lib.ptr(audio), batch,
            frames, ws.data_ptr(), nbytes, _lib.stream()), [audio]
    check_entry(
        device, lib.pm_vocos_head_workspace_bytes(_lib.PM_F16, batch, frames),
        call)


@pytest.fixture(scope='module')
def vocos_engine(device):
    """A finalized one-layer f16 engine; (handle, generator of its seed)"""
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(8)
    handle = ctypes.c_void_p()
    _lib.check(lib.pm_vocos_create(
        80, 256, 512, 1536, 1, 1024, 256, _lib.PM_F16, ctypes.byref(handle)))
    for name, tensor in vocos_state(gen, device, 1).items():
        _lib.check(lib.pm_vocos_load_tensor(
            handle, name.encode(), _lib.ptr(tensor),
            _lib.shape_array(tensor.shape), tensor.ndim, _lib.stream()))
    _lib.check(lib.pm_vocos_finalize(handle, _lib.stream()))
    torch.cuda.synchronize()
    yield handle, gen
    lib.pm_vocos_destroy(handle)


@pytest.mark.parametrize('ragged', [False, True])
def test_vocos_forward(device, vocos_engine, ragged):
    lib = _lib.lib()
    handle, gen = vocos_engine
    batch, frames = 2, 8
    features = randn(gen, device, batch, 80, frames)
    g = randn(gen, device, batch, 256)
    lengths = torch.tensor([8, 5], dtype=torch.int32, device=device)

    def call(ws, nbytes):
        audio = torch.zeros(batch, frames * 256, device=device)
        tail = (_lib.ptr(audio), batch, frames, ws.data_ptr(), nbytes,
                _lib.stream())
        if ragged:
            return lib.pm_vocos_forward_ragged(
                handle, _lib.ptr(features), _lib.ptr(g), batch,
                _lib.ptr(lengths, torch.int32), *tail), [audio]
        return lib.pm_vocos_forward(
            handle, _lib.ptr(features), _lib.ptr(g), batch, *tail), [audio]
    sizing = lib.pm_vocos_ragged_workspace_bytes if ragged \
        else lib.pm_vocos_workspace_bytes
    check_entry(device, sizing(handle, batch, frames), call)


@pytest.mark.parametrize('storage', ['f16', 'fp32'])
def test_fargan_forward(device, storage):
    """Both storage modes on the cluster kernels: fp32 storage places the
    conditioning behind the cluster state, and pm_fargan_check reads the
    error word between the two."""
    lib = _lib.lib()
    torch.manual_seed(9)
    model = promonet_amd.model.FARGAN(113, 258)
    model.weight_dtype = storage
    model = model.to(device).eval()
    handle = model.engine()
    gen = torch.Generator().manual_seed(10)
    batch, frames = 2, 2
    features = torch.randn(batch, 114, frames, generator=gen) * .3
    features[:, -1] = 100.      # the pitch period in samples
    features = features.to(device).contiguous()
    g = randn(gen, device, batch, 258)
    _lib.check(lib.pm_fargan_set_mode(handle, 2))

    def call(ws, nbytes):
        out = torch.zeros(batch, 1, frames * 256, device=device)
        code = lib.pm_fargan_forward(
            handle, _lib.ptr(features), 0, _lib.ptr(g), batch, None, 1,
            _lib.ptr(out), batch, frames, ws.data_ptr(), nbytes,
            _lib.stream())
        if code == 0:
            _lib.check(lib.pm_fargan_check(
                handle, batch, frames, ws.data_ptr(), _lib.stream()))
        return code, [out]
    check_entry(
        device, lib.pm_fargan_workspace_bytes(handle, batch, frames), call)


def test_hifigan_forward(device, golden_small):
    """The small configuration with the walks forced, which puts their
    scratch behind the activation buffers."""
    lib = _lib.lib()
    promonet_amd.configure(COMPUTE_DTYPE='f16', **golden_small['config'])
    try:
        torch.manual_seed(11)
        model = promonet_amd.model.HiFiGAN(
            promonet_amd.NUM_FEATURES, promonet_amd.GLOBAL_CHANNELS)
        model = model.to(device).eval()
        handle = model.engine()
        gen = torch.Generator().manual_seed(12)
        batch, frames = 1, 16
        features = randn(gen, device, batch, promonet_amd.NUM_FEATURES, frames)
        g = randn(gen, device, batch, promonet_amd.GLOBAL_CHANNELS)

        def call(ws, nbytes):
            out = torch.zeros(batch, 1, frames * 256, device=device)
            return lib.pm_hifigan_forward(
                handle, _lib.ptr(features), _lib.ptr(g), batch, _lib.ptr(out),
                batch, frames, ws.data_ptr(), nbytes, _lib.stream()), [out]
        _lib.check(lib.pm_debug_force(2, 0))
        size = lib.pm_hifigan_workspace_bytes(handle, batch, frames)
        assert size > lib.pm_walk_scratch_bytes(batch)
        check_entry(device, size, call)
    finally:
        _lib.check(lib.pm_debug_force(0, 0))
        promonet_amd.configure(
            HIFIGAN_UPSAMPLE_INITIAL_SIZE=512,
            COMPUTE_DTYPE=promonet_amd.config.DEFAULT_COMPUTE_DTYPE)


def audio(gen, device, batch, samples):
    return randn(gen, device, batch, samples, scale=.1)


def test_stft_mel(device):
    """pm_stft_mel_prepare fills the buffer (table, values), pm_stft_mel finds
    both in it again."""
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(13)
    mels, batch, samples = 80, 2, 4096
    basis = promonet_amd.preprocess.spectrogram.mel_basis().to(
        device=device, dtype=torch.float32).contiguous()
    assert basis.shape == (mels, 513)
    x = audio(gen, device, batch, samples)
    size = lib.pm_stft_mel_scratch_bytes(mels)

    def call(ws, nbytes):
        out = torch.zeros(batch, mels, samples // 256, device=device)
        code = lib.pm_stft_mel_prepare(
            _lib.ptr(basis), mels, ws.data_ptr(), nbytes, _lib.stream())
        if code == 0:
            _lib.check(lib.pm_stft_mel(
                _lib.ptr(x), ws.data_ptr(), _lib.ptr(out), batch, samples,
                mels, 1, 1e-5, _lib.stream()))
        return code, [out]
    check_entry(device, size, call)


def test_stft_magnitude_backward(device):
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(14)
    batch, samples = 2, 4096
    x = audio(gen, device, batch, samples)
    grad_out = randn(gen, device, batch, 513, samples // 256)

    def call(ws, nbytes):
        grad = torch.zeros_like(x)
        return lib.pm_stft_magnitude_backward(
            _lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(grad), batch, samples,
            ws.data_ptr(), nbytes, _lib.stream()), [grad]
    check_entry(
        device, lib.pm_stft_backward_scratch_bytes(batch, samples), call)


def test_loudness_single_pass(device):
    """The optimistic schedule: the one that keeps every group's minimum next
    to its maximum."""
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(15)
    batch, samples, bands = 2, 4096, 8
    x = audio(gen, device, batch, samples)
    x[1, 2048:] = 0.    # (a stretch on the floor: groups that are redone)
    weights = promonet_amd.preprocess.loudness.perceptual_weights_tensor(
        device)

    def call(ws, nbytes):
        out = torch.zeros(batch, bands, samples // 256, device=device)
        return lib.pm_loudness(
            _lib.ptr(x), _lib.ptr(weights), _lib.ptr(out), batch, samples,
            bands, promonet_amd.MIN_DB, ws.data_ptr(), nbytes,
            _lib.stream()), [out]
    try:
        _lib.check(lib.pm_stft_set_loudness_passes(1))
        check_entry(
            device, lib.pm_loudness_scratch_bytes(batch, samples), call)
    finally:
        _lib.check(lib.pm_stft_set_loudness_passes(2))


@pytest.mark.parametrize('with_gradient', [0, 1])
def test_sc_forward(device, with_gradient):
    """The sums and, with the gradient, the spectrum the entry leaves at the
    head of the workspace for pm_sc_adjoint."""
    from promonet_amd import loss
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(16)
    batch, samples, fft_size, hop_size = 3, 4096, 2560, 640
    x = audio(gen, device, batch, samples)
    y = audio(gen, device, batch, samples)
    window = loss._named_window(device, 'hann_window', fft_size, fft_size)
    twiddle = loss._twiddle(device, fft_size)
    size = lib.pm_sc_forward_workspace_bytes(
        batch, samples, fft_size, hop_size, with_gradient)
    partials = lib.pm_sc_forward_workspace_bytes(
        batch, samples, fft_size, hop_size, 0)

    def call(ws, nbytes):
        sums = torch.zeros(3, device=device)
        code = lib.pm_sc_forward(
            _lib.ptr(x), _lib.ptr(y), _lib.ptr(window), _lib.ptr(twiddle),
            _lib.ptr(sums), batch, samples, fft_size, hop_size, with_gradient,
            ws.data_ptr(), nbytes, _lib.stream())
        return code, [sums, ws[:size - partials].clone()]
    check_entry(device, size, call)
