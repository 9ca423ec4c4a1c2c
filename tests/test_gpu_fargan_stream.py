"""FARGAN streaming on the GPU: `step` / `stream` from a carried recurrent
state against the REAL reference's `FARGAN.step` (tests/golden/fargan_step.pt,
scripts/make_golden_fargan_step.py), and chunked synthesis equal to one
`forward` over the whole utterance, bit for bit."""
from pathlib import Path

import pytest
import torch

import fargan_step_oracle
import restatement as oracle
from util import check, max_abs

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / 'golden'
SIZES = (256, 256, 256, 260)
# fp32 math everywhere; the storage of the streamed weights differs. Gates
# <= 3x what MI355X measures on the reference's step goldens, worst of the
# warm-up, warm and random-state cases: audio fp32 3.4e-7, mixed 2.0e-5
# (random state), f16 6.5e-5; the returned states (GRU states in (-1, 1),
# conditioning outputs: O(1) where the audio is O(0.1)) fp32 2.9e-6, mixed
# 3.6e-5, f16 5.3e-4; the storage rounding is separated out in
# test_gpu_fargan_probe.py
GATE = {'fp32': 1e-6, 'f16': 1.9e-4, 'mixed': 6e-5}
STATE_GATE = {'fp32': 8e-6, 'f16': 1.5e-3, 'mixed': 1e-4}


@pytest.fixture(scope='module')
def step_golden():
    return torch.load(GOLDEN / 'fargan_step.pt', weights_only=False)


@pytest.fixture(scope='module')
def fargan(golden_fargan, golden_default, device):
    """build(dtype) -> promonet_amd.model.FARGAN with the weights of
    oracle.random_state_fargan(golden seed) on the device."""
    import promonet_amd
    state = oracle.random_state_fargan(seed=golden_fargan['seed'])
    state['pitch_distribution'] = golden_default['pitch_distribution'].clone()
    weights = {k[len('model.'):]: v for k, v in state.items()
               if k.startswith('model.')}
    models = {}

    def build(dtype, mode=0):
        if dtype not in models:
            model = promonet_amd.model.FARGAN(113, 258)
            model.load_state_dict(weights)
            model.weight_dtype = dtype
            models[dtype] = model.to(device).eval()
        models[dtype].kernel_mode = mode
        return models[dtype]
    build.state = state
    return build


@pytest.fixture(scope='module')
def utterances(fargan):
    """37 utterances x 172 frames of features (B, 114, T) and globals."""
    return fargan_step_oracle.features(37, 172, fargan.state, seed=71)


def split(states):
    return tuple(states.split(SIZES, dim=1))


def chunked(model, features, g, chunk, previous=None, states=None):
    pieces = []
    for start in range(0, features.shape[2], chunk):
        audio, previous, states = model.stream(
            features[..., start:start + chunk], g, previous, states)
        pieces.append(audio)
    return torch.cat(pieces, dim=2), previous, states


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', ['fp32', 'mixed', 'f16'])
def test_step_and_stream_match_reference(
    device, fargan, step_golden, dtype, mode
):
    """(a) a warm-up from zero state, then a chunk from the state it ended
    in; (b) a random state. Audio, previous samples and states."""
    model = fargan(dtype, mode)
    warm = int(step_golden['warm_frames'])
    audio_errors, state_errors = {}, {}
    for case in ('warm', 'random'):
        features = step_golden[f'{case}/features'].to(device)
        g = step_golden[f'{case}/global'].to(device)
        previous = step_golden[f'{case}/previous'].to(device)
        states = split(step_golden[f'{case}/states'].to(device))
        if case == 'warm':
            with torch.inference_mode():
                _, p0, s0 = model.stream(features[..., :warm], g)
            state_errors['warm-up'] = max_abs(
                torch.cat(s0, 1), step_golden['warm/states'])
            audio_errors['warm-up'] = max_abs(p0, previous)
            features = features[..., warm:]
        want_audio = step_golden[f'{case}/audio']
        want_states = step_golden[f'{case}/states_out']
        with torch.inference_mode():
            audio, p1, s1 = model.stream(features, g, previous, states)
            frames, p2, s2 = [], previous, states
            for t in range(features.shape[2]):
                frame, p2, s2 = model.step(features[..., t], g, p2, s2)
                frames.append(frame)
        stepped = torch.cat(frames, dim=1)[:, None]
        assert audio.shape == want_audio.shape and p1.shape == p2.shape
        assert [tuple(t.shape) for t in s2] == [
            (features.shape[0], n) for n in SIZES]
        audio_errors[case] = max(
            max_abs(audio, want_audio),
            max_abs(p1, step_golden[f'{case}/previous_out']))
        state_errors[case] = max_abs(torch.cat(s1, 1), want_states)
        # one step at a time: the same bits as the chunk
        assert torch.equal(stepped, audio) and torch.equal(p2, p1)
        assert all(torch.equal(a, b) for a, b in zip(s1, s2))
    print(f'fargan step {dtype} mode {mode}: audio {audio_errors}, '
          f'states {state_errors}')
    for case, error in audio_errors.items():
        check(error, GATE[dtype], f'fargan_step_audio:{dtype}', case)
    for case, error in state_errors.items():
        check(error, STATE_GATE[dtype], f'fargan_step_states:{dtype}', case)


@pytest.mark.parametrize('batch', [3, 37])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', ['fp32', 'mixed', 'f16'])
def test_chunking_is_exact(device, fargan, utterances, dtype, mode, batch):
    """40 frames streamed in chunks of 1, 7, 13 and 19 frames with carried
    state == forward over all 40, bit for bit (mode 2, batch 37: two
    utterances per cluster in lockstep and a padded slot); the final state
    does not depend on the chunking."""
    model = fargan(dtype, mode)
    features = utterances[0][:batch, :, :40].to(device)
    g = utterances[1][:batch].to(device)
    with torch.inference_mode():
        want = model(features, g[..., None], None)
        whole, p_whole, s_whole = model.stream(features, g)
        assert torch.equal(whole, want)
        for chunk in (1, 7, 13, 19):
            got, previous, states = chunked(model, features, g, chunk)
            assert torch.equal(got, want), chunk
            assert torch.equal(previous, p_whole), chunk
            assert all(torch.equal(a, b) for a, b in zip(states, s_whole))
    assert torch.equal(p_whole[:, 0], want[:, 0, -512:])


@pytest.mark.parametrize('mode', [1, 2])
def test_step_equals_forward(device, fargan, utterances, mode):
    """Twelve successive step() calls == forward on 12 frames."""
    from promonet_amd.model import initialize_recurrent_state
    model = fargan('fp32', mode)
    features = utterances[0][:2, :, :12].to(device)
    g = utterances[1][:2].to(device)
    previous = torch.rand(2, 1, 512, generator=torch.Generator().manual_seed(
        3)).to(device) * .2 - .1
    states = initialize_recurrent_state(2, device)
    frames = []
    with torch.inference_mode():
        want = model(features, g[..., None], previous)
        for t in range(12):
            frame, previous, states = model.step(
                features[:, :, t], g[..., None], previous, states)
            assert frame.shape == (2, 256) and previous.shape == (2, 1, 512)
            frames.append(frame)
    assert torch.equal(torch.cat(frames, dim=1)[:, None], want)


@pytest.mark.parametrize('mode', [1, 2])
def test_zero_state_equals_forward_and_oracle(device, fargan, utterances, mode):
    """stream(states=None) == forward; its returned states match the
    oracle's after the same frames."""
    model = fargan('fp32', mode)
    features, g = utterances[0][:3, :, :10], utterances[1][:3]
    previous = torch.zeros(3, 1, 512)
    with torch.inference_mode():
        want = model(features.to(device), g[..., None].to(device), None)
        got, p, states = model.stream(
            features.to(device), g.to(device), previous.to(device))
        _, want_states, want_previous = oracle.fargan_forward(
            features, g[..., None], previous, fargan.state, return_states=True)
    assert torch.equal(got, want)
    check(max_abs(torch.cat(states, 1), torch.cat(want_states, 1)),
          STATE_GATE['fp32'], 'fargan_step_states:fp32', 'zero state')
    check(max_abs(p[:, 0], want_previous), GATE['fp32'],
          'fargan_step_audio:fp32', 'zero state')


@pytest.mark.parametrize('mode', [1, 2])
def test_long_run_in_chunks(device, fargan, utterances, mode):
    """Batch 4, 172 frames in 43-frame chunks == forward."""
    model = fargan('fp32', mode)
    features = utterances[0][4:8].to(device)
    g = utterances[1][4:8].to(device)
    with torch.inference_mode():
        want = model(features, g[..., None], None)
        got, previous, _ = chunked(model, features, g, 43)
    assert got.shape == (4, 1, 172 * 256)
    assert torch.equal(got, want)
    assert torch.equal(previous[:, 0], want[:, 0, -512:])


def test_behaviour(device, fargan, step_golden):
    """Deterministic; the two kernels' final states agree; bad shapes,
    batch mismatches, host tensors and overlapping outputs are rejected."""
    from promonet_amd import _lib
    model = fargan('fp32', 2)
    features = step_golden['random/features'].to(device)
    g = step_golden['random/global'].to(device)
    previous = step_golden['random/previous'].to(device)
    states = split(step_golden['random/states'].to(device))
    with torch.inference_mode():
        a = model.stream(features, g, previous, states)
        b = model.stream(features, g, previous, states)
        model.kernel_mode = 1
        c = model.stream(features, g, previous, states)
    model.kernel_mode = 0
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert max_abs(torch.cat(a[2], 1), torch.cat(c[2], 1)) < 2e-6
    assert max_abs(a[0], c[0]) < 2e-6
    with torch.inference_mode():
        with pytest.raises(ValueError):                       # no period
            model.stream(features[:, :-1], g, previous, states)
        with pytest.raises(ValueError):                       # state batch
            model.stream(features, g, previous, [s[:2] for s in states])
        with pytest.raises(ValueError):                       # state width
            model.stream(features, g, previous, states[:3] + (states[0],))
        with pytest.raises(ValueError):                       # three states
            model.step(features[..., 0], g, previous, states[:3])
        with pytest.raises(ValueError):
            model.step(features[..., 0], g[:2], previous, states)
        with pytest.raises(RuntimeError):
            model.step(features[..., 0], g, previous,
                       tuple(s.cpu() for s in states))
        with pytest.raises(RuntimeError):
            model.stream(features.cpu(), g.cpu())
    # through the C entry: an output that overlaps an input
    lib = _lib.lib()
    engine = model.engine()
    batch, frames = features.shape[0], features.shape[2]
    x = features.contiguous()
    flat = step_golden['random/states'].to(device).contiguous()
    out = torch.empty(batch, 1, frames * 256, device=device)
    prev_out = torch.empty(batch, 512, device=device)
    states_out = torch.empty(batch, 1028, device=device)
    size = lib.pm_fargan_workspace_bytes(engine, batch, frames)
    ws = torch.empty(size, dtype=torch.uint8, device=device)

    def call(out_, prev_, states_, states_in=flat):
        return lib.pm_fargan_forward_stateful(
            engine, _lib.ptr(x), 0, _lib.ptr(g), batch,
            _lib.ptr(previous.reshape(batch, 512)), batch,
            _lib.ptr(states_in), _lib.ptr(out_), _lib.ptr(prev_),
            _lib.ptr(states_), batch, frames, ws.data_ptr(), ws.numel(),
            _lib.stream())
    assert call(out, prev_out, flat) == _lib.PM_EINVAL          # states in-place
    assert call(out, prev_out, x) == _lib.PM_EINVAL             # over features
    assert call(out, out.view(-1)[:512 * batch],
                states_out) == _lib.PM_EINVAL                   # outputs overlap
    _lib.check(lib.pm_fargan_set_mode(engine, 2))
    assert call(out, prev_out, states_out) == 0
    _lib.check(lib.pm_fargan_check(engine, batch, frames, ws.data_ptr(),
                                   _lib.stream()))
    assert torch.equal(out, a[0]) and torch.equal(prev_out, a[1][:, 0])
    assert torch.equal(states_out, torch.cat(a[2], 1))
