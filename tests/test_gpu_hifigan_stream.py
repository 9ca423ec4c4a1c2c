"""HiFi-GAN streaming on the GPU: chunks in, audio out, and
the concatenated audio equals one `forward` over the concatenated frames BIT
FOR BIT - every operand type, every schedule edge, eager and as replayed
graphs, at the vocoder and at the Generator level. The comparison is
`hifigan_stream_oracle.same`, which tests/test_cpu_hifigan_stream.py shows to
reject a short context, a shifted emit, a misplaced history and a missing
`finish`."""
import pytest
import torch

import hifigan_stream_oracle as stream_oracle
import restatement as oracle
from promonet_amd.model import HiFiGANStream, stream_schedule

pytestmark = pytest.mark.gpu

# every sequence runs over 70 frames, but the one with the single-frame
# pushes, whose chunks add up to 83: it runs over its own 83
FRAMES = 70
LONGEST = 83
HOP = 256
# a chunk below the lookahead (the first pushes emit nothing), equal to the
# context, longer than the history; windows that are not yet full
SEQUENCES = ([70], [1] * 16 + [3, 13, 14, 27, 10], [8] * 8 + [6],
             [13] * 5 + [5], [40, 30], [27, 1, 42])
MODES = ('bf16', 'f16', 'checkpoint', 'fp32')


@pytest.fixture(scope='module')
def default_state(golden_default):
    state = oracle.random_state(seed=golden_default['seed'])
    state['pitch_distribution'] = golden_default['pitch_distribution'].clone()
    return state


@pytest.fixture(scope='module')
def models(default_state, device):
    """build(dtype) -> the Generator of that operand type, made once"""
    import promonet_amd
    made = {}

    def build(dtype):
        if dtype not in made:
            promonet_amd.configure(COMPUTE_DTYPE=dtype)
            try:
                model = promonet_amd.model.Generator()
            finally:
                promonet_amd.configure(
                    COMPUTE_DTYPE=promonet_amd.config.DEFAULT_COMPUTE_DTYPE)
            model.load_state_dict(default_state)
            made[dtype] = model.to(device).eval()
        return made[dtype]
    return build


@pytest.fixture(scope='module')
def inputs(device):
    """Three utterances of LONGEST frames: forward()'s arguments"""
    return [t.to(device) for t in oracle.synthetic_inputs(3, LONGEST, seed=41)]


def cut(inputs, batch, frames=FRAMES):
    """The first `frames` frames of the first `batch` utterances"""
    return [(t[:batch, ..., :frames] if t.ndim > 1 else t[:batch]).contiguous()
            for t in inputs]


def conditioning(model, inputs, batch, frames=FRAMES):
    """features (B, 113, T), channels-last features (B, T, 128), globals"""
    rows = cut(inputs, batch, frames)
    with torch.inference_mode():
        return (model.prepare_features(*rows[:4]),
                model._features(*rows[:4], channels_last=True),
                model.prepare_global_features(*rows[4:]))


def run(stream, features, chunks, channels_last=False):
    """Every push's audio, then finish()'s: the first sum(chunks) frames"""
    audio, position = [], 0
    for chunk in chunks:
        piece = features[:, position:position + chunk] if channels_last \
            else features[..., position:position + chunk]
        audio.append(stream.push(piece, channels_last))
        position += chunk
    assert position in (FRAMES, LONGEST)
    audio.append(stream.finish())
    return audio


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('dtype', MODES)
def test_stream_equals_one_forward(models, inputs, dtype, batch):
    model = models(dtype)
    features, features_cl, g = conditioning(model, inputs, batch, LONGEST)
    vocoder = model.model
    assert vocoder.context() == (13, 13)
    with torch.inference_mode():
        full = {frames: vocoder(features[..., :frames].contiguous(), g)
                for frames in (FRAMES, LONGEST)}
        assert full[FRAMES].shape == (batch, 1, FRAMES * HOP)
        assert torch.equal(
            vocoder.forward_channels_last(features_cl, g), full[LONGEST])
        assert not torch.equal(
            full[FRAMES][..., -13 * HOP:],
            full[LONGEST][..., (FRAMES - 13) * HOP:FRAMES * HOP])
        for chunks in SEQUENCES:
            stream = vocoder.open_stream(g, batch)
            audio = run(stream, features, chunks)
            assert stream_oracle.same(audio, full[sum(chunks)]), \
                (dtype, batch, chunks)
            # what every push emits is what the schedule says
            seen = 0
            for chunk, piece in zip(chunks, audio):
                count = stream_schedule(seen, chunk, 13, 13)[2]
                assert piece.shape == (batch, 1, count * HOP)
                seen += chunk
            assert audio[-1].shape[-1] == 13 * HOP
        # channels-last chunks (what pm_prepare_features writes)
        stream = vocoder.open_stream(g, batch)
        assert stream_oracle.same(
            run(stream, features_cl, SEQUENCES[2], channels_last=True),
            full[FRAMES])


def test_c_context_matches_the_mirror(models):
    import ctypes
    from promonet_amd import _lib
    vocoder = models('f16').model
    left, right = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().pm_hifigan_context(
        vocoder.engine(), ctypes.byref(left), ctypes.byref(right)))
    assert (left.value, right.value) == vocoder.context() == (13, 13)


@pytest.mark.parametrize('lookahead', [0, 1, 12])
def test_reduced_lookahead_is_the_truncated_forward(models, inputs, lookahead):
    """With fewer frames held back than the right context, a push emits what
    `forward` gives for the utterance that ends where the stream has got to"""
    model = models('checkpoint')
    features, _, g = conditioning(model, inputs, 2, LONGEST)
    vocoder = model.model
    with torch.inference_mode():
        for chunks in (SEQUENCES[1], SEQUENCES[4]):
            full = vocoder(features[..., :sum(chunks)].contiguous(), g)
            stream = vocoder.open_stream(g, 2, lookahead=lookahead)
            audio = run(stream, features, chunks)
            seen, position = 0, 0
            for chunk, piece in zip(chunks, audio):
                seen += chunk
                emitted = piece.shape[-1]
                assert emitted == HOP * (
                    max(0, seen - lookahead) - max(0, seen - chunk - lookahead))
                if emitted:
                    want = vocoder(features[..., :seen].contiguous(), g)
                    assert torch.equal(
                        piece, want[..., position:position + emitted]), \
                        (lookahead, chunks, seen)
                position += emitted
            assert audio[-1].shape[-1] == lookahead * HOP
            assert torch.equal(audio[-1], full[..., position:])
            # and it is NOT the full forward (lookahead 12: frames 13 away
            # reach the audio with weights too small to show at every push)
            if lookahead < 12:
                assert not stream_oracle.same(audio, full)


def test_rows_are_independent(models, inputs):
    model = models('bf16')
    features, _, g = conditioning(model, inputs, 3)
    vocoder = model.model
    chunks = SEQUENCES[3]
    with torch.inference_mode():
        together = torch.cat(
            run(vocoder.open_stream(g, 3), features, chunks), dim=-1)
        for row in range(3):
            alone = torch.cat(run(
                vocoder.open_stream(g[row:row + 1], 1),
                features[row:row + 1], chunks), dim=-1)
            assert torch.equal(alone, together[row:row + 1]), row
        # one global row broadcast over the batch
        shared = torch.cat(run(
            vocoder.open_stream(g[:1], 3), features, chunks), dim=-1)
        assert torch.equal(shared[:1], together[:1])
        assert not torch.equal(shared[1:], together[1:])


def test_nothing_outside_the_history_is_read(models, inputs):
    """Window buffers full of NaN give the same bits"""
    model = models('f16')
    features, _, g = conditioning(model, inputs, 2, LONGEST)
    vocoder = model.model
    with torch.inference_mode():
        for chunks in SEQUENCES[1:4]:
            full = vocoder(features[..., :sum(chunks)].contiguous(), g)
            stream = vocoder.open_stream(g, 2)
            for index in (0, 1):
                stream._window(index, 128).fill_(float('nan'))
            buffers = [w.data_ptr() for w in stream._windows]
            audio = run(stream, features, chunks)
            assert [w.data_ptr() for w in stream._windows] == buffers
            assert stream_oracle.same(audio, full), chunks
            assert torch.isnan(stream._windows[0][:, -1]).all()


def test_reset_and_two_streams_on_one_module(models, inputs):
    model = models('checkpoint')
    features, _, g = conditioning(model, inputs, 2)
    vocoder = model.model
    chunks = SEQUENCES[2]
    with torch.inference_mode():
        full = vocoder(features, g)
        stream = vocoder.open_stream(g, 2)
        first = run(stream, features, chunks)
        with pytest.raises(ValueError):
            stream.push(features[..., :8])
        with pytest.raises(ValueError):
            stream.finish()
        stream.reset()
        again = run(stream, features, chunks)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        assert stream_oracle.same(again, full)
        # a reset in the middle of an utterance
        stream.reset()
        stream.push(features[..., :30])
        stream.reset()
        assert stream_oracle.same(run(stream, features, chunks), full)

        # two streams, pushes interleaved, the second one utterance 1 alone
        # with other chunks; a plain forward in between
        one = vocoder.open_stream(g, 2)
        two = vocoder.open_stream(g[1:], 1, lookahead=13)
        got_one, got_two, at_one, at_two = [], [], 0, 0
        other = SEQUENCES[3]
        for step in range(max(len(chunks), len(other))):
            if step < len(chunks):
                got_one.append(one.push(
                    features[..., at_one:at_one + chunks[step]]))
                at_one += chunks[step]
            if step == 3:
                assert torch.equal(vocoder(features, g), full)
            if step < len(other):
                got_two.append(two.push(
                    features[1:, :, at_two:at_two + other[step]]))
                at_two += other[step]
        got_one.append(one.finish())
        got_two.append(two.finish())
        assert stream_oracle.same(got_one, full)
        assert stream_oracle.same(got_two, full[1:])


@pytest.mark.parametrize('dtype', ['bf16', 'checkpoint'])
def test_graph_mode(models, inputs, dtype):
    """graph=True: the first step of a (keep, chunk) shape runs eagerly, later
    ones replay a captured graph; a stream of equal chunks settles on two
    graphs, one per buffer phase."""
    model = models(dtype)
    features, _, g = conditioning(model, inputs, 1)
    vocoder = model.model
    chunks = SEQUENCES[2]
    with torch.inference_mode():
        full = vocoder(features, g)
        eager = run(vocoder.open_stream(g, 1), features, chunks)
    assert stream_oracle.same(eager, full)
    # outside inference mode and inside
    for inside in (False, True):
        stream = vocoder.open_stream(g, 1, graph=True)
        sizes, audio, position = [], [], 0
        with torch.inference_mode(inside):
            for chunk in chunks:
                audio.append(stream.push(
                    features[..., position:position + chunk]))
                position += chunk
                sizes.append(len(stream._graphs))
            audio.append(stream.finish())
        assert all(torch.equal(a, b) for a, b in zip(audio, eager)), inside
        # pushes 0-3 fill the history (keep 0, 8, 16, 24: four shapes, eager);
        # push 4 is the first with keep 26 (eager: its previous window is the
        # short one of push 3), pushes 5 and 6 capture the two phases, push 7
        # replays, push 8 (6 frames) is a new shape
        assert sizes == [0, 0, 0, 0, 0, 1, 2, 2, 2], sizes
        # the same utterance again: every steady push replays; other inputs
        # give other audio
        stream.reset()
        flipped = features.flip(-1).contiguous()
        with torch.inference_mode():
            want = vocoder(flipped, g)
        with torch.inference_mode(inside):
            again = run(stream, flipped, chunks)
        assert stream_oracle.same(again, want)
        assert not torch.equal(again[7], audio[7])
        assert len(stream._graphs) <= HiFiGANStream.MAX_PACKED_GRAPHS
    # a long steady state: no capture after the second one, and at most
    # MAX_PACKED_GRAPHS graphs however many shapes come by
    stream = vocoder.open_stream(g, 1, lookahead=0, graph=True)
    sizes = []
    with torch.inference_mode():
        for start in range(0, 64, 4):
            stream.push(features[..., start:start + 4])
            sizes.append(len(stream._graphs))
        assert sizes[-1] == 2 and sizes[6:] == [2] * 10, sizes
        stream.reset()
        for chunk in (1, 2, 3, 5, 6, 7) * 3:
            stream.push(features[..., :chunk])
            assert len(stream._graphs) <= HiFiGANStream.MAX_PACKED_GRAPHS
    # a larger eager forward in between re-allocates the shared workspace;
    # the graphs own theirs
    stream = vocoder.open_stream(g, 1, graph=True)
    with torch.inference_mode():
        audio = [stream.push(features[..., s:s + 8]) for s in range(0, 56, 8)]
        big = [t.to(features.device) for t in oracle.synthetic_inputs(2, 300)]
        model(*big, None)
        audio += [stream.push(features[..., 56:64]),
                  stream.push(features[..., 64:]), stream.finish()]
    assert stream_oracle.same(audio, full)


def test_generator_level(models, inputs):
    import promonet_amd
    model = models('bf16')
    rows = cut(inputs, 2, LONGEST)
    with torch.inference_mode():
        full = model(*rows, None)
        # Generator.open_stream
        stream = model.open_stream(*rows[4:])
        audio, position = [], 0
        for chunk in SEQUENCES[1]:
            audio.append(stream.push(
                *[t[..., position:position + chunk] for t in rows[:4]]))
            position += chunk
        audio.append(stream.finish())
        assert stream_oracle.same(audio, full)
        with pytest.raises(ValueError):
            stream.push(*[t[..., :4] for t in rows[:4]])

        # packed_stream against packed_inference
        rows = cut(inputs, 2)
        packed = model.pack_features(
            rows[0], rows[1][:, None], rows[2][:, None], *rows[3:]).clone()
        want = model.packed_inference(packed)
        for graph in (False, True):
            stream = model.packed_stream(graph=graph)
            audio, position = [], 0
            for chunk in SEQUENCES[2]:
                audio.append(stream.push(
                    packed[..., position:position + chunk].contiguous()))
                position += chunk
            audio.append(stream.finish())
            assert stream_oracle.same(audio, want), graph
        with pytest.raises(ValueError):
            stream.push(packed[:1, :, :8].contiguous())     # another batch
        with pytest.raises(ValueError):
            stream.push(packed[:, :50, :8].contiguous())    # not 53 channels

    # from_features(chunk_frames=16) against the unchunked call
    promonet_amd.synthesize.set_model(model, rows[1].device)
    one = [t[:1] for t in rows[:4]]
    want = promonet_amd.synthesize.from_features(*one, speaker=5, gpu=0)
    got = promonet_amd.synthesize.from_features(
        *one, speaker=5, gpu=0, chunk_frames=16)
    assert want.shape == (1, FRAMES * HOP)
    assert got.shape == want.shape and torch.equal(got, want)
    got = promonet_amd.synthesize.from_features(
        *one, speaker=5, gpu=0, chunk_frames=FRAMES + 9)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        promonet_amd.synthesize.from_features(
            *one, speaker=5, gpu=0, chunk_frames=0)


def test_value_errors(models, inputs):
    import promonet_amd
    model = models('f16')
    features, features_cl, g = conditioning(model, inputs, 2)
    vocoder = model.model
    with pytest.raises(ValueError):
        vocoder.open_stream(g, 2, lookahead=14)
    with pytest.raises(ValueError):
        vocoder.open_stream(g, 2, lookahead=-1)
    with pytest.raises(ValueError):
        vocoder.open_stream(g, 3)                 # two global rows, batch 3
    with pytest.raises(ValueError):
        vocoder.open_stream(g[..., :100, :], 2)   # not 258 global channels
    stream = vocoder.open_stream(g, 2)
    with pytest.raises(ValueError):
        stream.push(features[:1, :, :8])          # another batch
    with pytest.raises(ValueError):
        stream.push(features[:, :100, :8])        # not 113 channels
    with pytest.raises(ValueError):
        stream.push(features[..., :8], channels_last=True)
    with pytest.raises(ValueError):
        stream.push(features_cl[:, :8, :64], channels_last=True)
    assert stream.seen == 0
    assert stream.push(features[..., :0]).shape == (2, 1, 0)
    stream.push(features[..., :20])
    stream.finish()
    with pytest.raises(ValueError):
        stream.push(features[..., 20:28])
    with pytest.raises(ValueError):
        stream.finish()
    # FARGAN carries a recurrent state instead
    promonet_amd.configure(MODEL='fargan')
    try:
        fargan = promonet_amd.model.Generator()
    finally:
        promonet_amd.configure(MODEL='hifigan')
    with pytest.raises(ValueError, match='FARGAN.stream'):
        fargan.open_stream(inputs[4], inputs[5], inputs[6])
    with pytest.raises(ValueError, match='FARGAN.stream'):
        fargan.packed_stream()
