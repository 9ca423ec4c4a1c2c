"""Generate the committed golden vectors under tests/golden/ by importing the
REAL reference (`/root/reference/promonet`, stubbed third-party deps) in the
build container, and check the CPU restatement against it while doing so.

TEST INFRASTRUCTURE ONLY - runs only where /root/reference exists:

    python oracle/make_golden.py            # both configs (two subprocesses)

Fixtures are data: inputs, reference-constructed weights (small config only)
and the reference's outputs. No reference source is copied.
"""
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden'
sys.path.insert(0, str(ROOT / 'oracle'))


def small_config_file():
    file = Path(tempfile.gettempdir()) / 'promonet_small_config.py'
    file.write_text(
        "MODULE = 'promonet'\nCONFIG = 'small'\n"
        "HIFIGAN_UPSAMPLE_INITIAL_SIZE = 64\n")
    return file


def variant_config_file(which):
    """Non-default conditioning variants reachable from the same forward
    (generator.py:35-38, 97-104, 140-147) on a tiny vocoder."""
    file = Path(tempfile.gettempdir()) / f'promonet_{which}_config.py'
    extra = {'zero_shot': 'ZERO_SHOT = True\n',
             'sparse_none': 'SPARSE_PPG_METHOD = None\n'}[which]
    file.write_text(
        f"MODULE = 'promonet'\nCONFIG = '{which}'\n"
        "HIFIGAN_UPSAMPLE_INITIAL_SIZE = 32\n" + extra)
    return file


def layout():
    """What `promonet_amd.patch(promonet)` reads and replaces in the reference
    package, as data: its upper-case constants (names only for the
    filesystem-valued ones), the kind of every attribute the patch swaps, and
    the size of `Generator().state_dict()`. tests/test_cpu_host.py rebuilds a
    stand-in package of this shape."""
    import json
    import reference_import

    promonet = reference_import.load()
    constants, opaque = {}, []
    for name in sorted(dir(promonet)):
        if not name.isupper():
            continue
        value = getattr(promonet, name)
        try:
            text = json.dumps(value)
        except TypeError:
            opaque.append(name)
            continue
        if '/' in text:
            opaque.append(name)
        else:
            constants[name] = value
    attributes = {}
    for path in (
            'model.Generator', 'model.HiFiGAN', 'model.FARGAN',
            'synthesize.core', 'preprocess.spectrogram.from_audio',
            'preprocess.spectrogram.linear_to_mel',
            'preprocess.loudness.from_audio') + tuple(
                f'synthesize{core}.{name}' for core in ('', '.core')
                for name in ('from_features', 'from_file', 'from_file_to_file',
                             'from_files_to_files', 'generate')):
        target = promonet
        for part in path.split('.'):
            target = getattr(target, part)
        attributes[path] = ('module' if isinstance(target, type(promonet))
                            else 'class' if isinstance(target, type)
                            else 'function')
    GOLDEN.mkdir(parents=True, exist_ok=True)
    (GOLDEN / 'reference_layout.json').write_text(json.dumps({
        'constants': constants,
        'opaque_constants': opaque,
        'attributes': attributes,
        'generator_state_dict_entries':
            len(promonet.model.Generator().state_dict())},
        indent=1, sort_keys=True) + '\n')


def run(which):
    import torch
    import reference_import
    import restatement as oracle

    if which == 'layout':
        layout()
        return

    configs = {
        'small': [small_config_file()],
        'zero_shot': [variant_config_file('zero_shot')],
        'sparse_none': [variant_config_file('sparse_none')],
        'fargan': [reference_import.REFERENCE_ROOT / 'config' / 'fargan.py'],
    }.get(which, [])
    promonet = reference_import.load(configs)
    torch.manual_seed(0)
    GOLDEN.mkdir(parents=True, exist_ok=True)

    if which == 'fargan':
        # config/fargan.py: frame-autoregressive GRU vocoder
        assert promonet.MODEL == 'fargan'
        assert promonet.NUM_PREVIOUS_SAMPLES == 512
        model = promonet.model.Generator().eval()
        reference_state = model.state_dict()
        state = oracle.random_state_fargan(seed=0)
        state['pitch_distribution'] = \
            reference_state['pitch_distribution'].clone()
        model.load_state_dict(state)
        golden = {
            'seed': 0,
            'state_keys': {
                k: tuple(v.shape) for k, v in reference_state.items()},
            'num_previous_samples': promonet.NUM_PREVIOUS_SAMPLES}
        gen = torch.Generator().manual_seed(2)
        for name, (batch, frames, seed) in {
            'b2_t8': (2, 8, 3), 'b1_t60': (1, 60, 4), 'b3_t25': (3, 25, 6)
        }.items():
            inputs = oracle.synthetic_inputs(batch, frames, seed=seed)
            previous = torch.rand(batch, 1, 512, generator=gen) * .2 - .1 \
                if name == 'b3_t25' else torch.zeros(batch, 1, 512)
            with torch.inference_mode():
                audio = model(*inputs, previous)
                features = model.prepare_features(*inputs[:4])
                mine = oracle.fargan_generator_forward(
                    *inputs, state, previous)
            error = (audio - mine).abs().max().item()
            print(f'fargan {name}: restatement vs reference {error:.3e}')
            assert error < 1e-6 and features.shape[1] == 114
            golden[name] = {
                'batch': batch, 'frames': frames, 'input_seed': seed,
                'previous': previous, 'audio': audio,
                'period': features[:, -1].clone()}
        torch.save(golden, GOLDEN / 'generator_fargan.pt')
        return

    if which == 'edit_voiced':
        # Selective time-stretch (edit/core.py:57-110): the REAL reference loop
        # over the restated phoneme inventory (third-party constants, see
        # reference_import). PPG rows follow that inventory's order.
        frames = 61
        inputs = oracle.synthetic_inputs(1, frames, seed=19)
        loud, pit, per, pg = (
            inputs[0][0], inputs[1], inputs[2], inputs[3][0])
        cases = []
        for ratio, unvoiced, silence, cents in (
            (1.4, False, True, None), (.7, False, False, 300.),
            (1.15, False, False, None)
        ):
            # (stretch_unvoiced=True, stretch_silence=False) cannot be pinned:
            # the reference extends its index list with phoneme STRINGS there
            # (edit/core.py:69-76) and torch.tensor(indices) raises
            result = promonet.edit.from_features(
                loud.clone(), pit.clone(), per.clone(), pg.clone(), cents,
                ratio, None, unvoiced, silence, return_grid=True)
            mine = oracle.edit_from_features(
                loud.clone(), pit.clone(), per.clone(), pg.clone(), cents,
                ratio, None, None, unvoiced, silence)
            mine_grid = oracle.grid_selective(
                pg, ratio, oracle.stretched_phonemes(unvoiced, silence))
            error = (mine_grid - result[4]).abs().max().item()
            print(f'edit_voiced ratio {ratio}: grid vs reference {error:.3e}')
            assert error < 1e-4
            for a, b in zip(result[:4], mine):
                assert a.shape == b.shape and (a - b).abs().max() < 1e-3
            cases.append({
                'time_stretch_ratio': ratio, 'stretch_unvoiced': unvoiced,
                'stretch_silence': silence, 'pitch_shift_cents': cents,
                'grid': result[4].clone(),
                'outputs': tuple(t.clone() for t in result[:4])})
        torch.save({'frames': frames, 'input_seed': 19, 'cases': cases},
                   GOLDEN / 'edit_voiced.pt')
        return

    if which in ('zero_shot', 'sparse_none'):
        assert promonet.HIFIGAN_UPSAMPLE_INITIAL_SIZE == 32
        model = promonet.model.Generator().eval()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        inputs = list(oracle.synthetic_inputs(2, 20, seed=23))
        if which == 'zero_shot':
            assert promonet.ZERO_SHOT and 'speaker_embedding.bias' in state
            gen = torch.Generator().manual_seed(29)
            inputs[4] = torch.randn(
                2, promonet.WAVLM_EMBEDDING_CHANNELS, generator=gen)
        else:
            assert promonet.SPARSE_PPG_METHOD is None
            assert 'ppg_threshold' not in state
        with torch.inference_mode():
            features = model.prepare_features(*inputs[:4])
            global_features = model.prepare_global_features(*inputs[4:7])
            audio = model(*inputs, model.default_previous_samples)
            # the restatement, fed the same conditioning variant
            mine_features = oracle.prepare_features(
                *inputs[:4], state['pitch_distribution'],
                state['pitch_embedding.weight'],
                state.get('ppg_threshold', 0.),
                'percentile' if which == 'zero_shot' else None)
            mine_global = oracle.prepare_global_features(
                *inputs[4:7], state['speaker_embedding.weight'],
                state.get('speaker_embedding.bias'))
            mine = oracle.hifigan_forward(mine_features, mine_global, state)
        assert (features - mine_features).abs().max() < 1e-6
        assert (global_features - mine_global).abs().max() < 1e-6
        error = (audio - mine).abs().max().item()
        print(f'{which}: restatement vs reference max-abs {error:.3e}')
        assert error < 1e-6
        torch.save({
            'config': {'HIFIGAN_UPSAMPLE_INITIAL_SIZE': 32,
                       'ZERO_SHOT': which == 'zero_shot',
                       'SPARSE_PPG_METHOD':
                           None if which == 'sparse_none' else 'percentile'},
            'state': state, 'inputs': inputs, 'features': features,
            'global_features': global_features, 'audio': audio},
            GOLDEN / f'variant_{which}.pt')
        return

    if which == 'small':
        assert promonet.HIFIGAN_UPSAMPLE_INITIAL_SIZE == 64
        model = promonet.model.Generator().eval()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        inputs = oracle.synthetic_inputs(2, 24, seed=11)
        with torch.inference_mode():
            features = model.prepare_features(*inputs[:4])
            global_features = model.prepare_global_features(*inputs[4:7])
            audio = model(*inputs, model.default_previous_samples)
            mine = oracle.generator_forward(*inputs, state)
        error = (audio - mine).abs().max().item()
        print(f'small: restatement vs reference max-abs {error:.3e}')
        assert error < 1e-6
        torch.save({
            'config': {'HIFIGAN_UPSAMPLE_INITIAL_SIZE': 64},
            'state': state,
            'inputs': inputs,
            'features': features,
            'global_features': global_features,
            'audio': audio}, GOLDEN / 'generator_small.pt')
        return

    # ---- default configuration ------------------------------------------
    model = promonet.model.Generator().eval()
    reference_state = model.state_dict()
    # weights regenerated from a seed on both sides (57 MB is too big to
    # commit): restatement-defined init, loaded INTO the reference module
    state = oracle.random_state(seed=0)
    state['pitch_distribution'] = reference_state['pitch_distribution'].clone()
    model.load_state_dict(state)
    golden = {'seed': 0, 'input_seed': 1234,
              'pitch_distribution': state['pitch_distribution'].clone()}

    for name, (batch, frames) in {'b2_t40': (2, 40), 'b1_t7': (1, 7)}.items():
        inputs = oracle.synthetic_inputs(batch, frames, seed=1234)
        with torch.inference_mode():
            audio = model(*inputs, model.default_previous_samples)
            mine = oracle.generator_forward(*inputs, state)
        error = (audio - mine).abs().max().item()
        print(f'{name}: restatement vs reference max-abs {error:.3e}')
        assert error < 1e-6
        golden[name] = {'batch': batch, 'frames': frames, 'audio': audio}

    # synthesize.from_features through the reference's public API (B = 1)
    promonet.synthesize.generate.model = model
    promonet.synthesize.generate.checkpoint = None
    promonet.synthesize.generate.device = torch.device('cpu')
    inputs = oracle.synthetic_inputs(1, 12, seed=99)
    api = promonet.synthesize.from_features(
        inputs[0][0], inputs[1], inputs[2], inputs[3], speaker=3,
        spectral_balance_ratio=1.25, loudness_ratio=.8)
    mine = oracle.from_features(
        inputs[0][0], inputs[1], inputs[2], inputs[3], state, 3, 1.25, .8)
    assert api.shape == (1, 12 * 256) and (api - mine).abs().max() < 1e-6
    golden['from_features'] = {
        'frames': 12, 'input_seed': 99, 'speaker': 3,
        'spectral_balance_ratio': 1.25, 'loudness_ratio': .8, 'audio': api}

    # prepare_features: 8-row and 513-row loudness
    inputs = oracle.synthetic_inputs(2, 24, seed=5)
    wide = oracle.synthetic_inputs(2, 24, seed=5, loudness_rows=513)[0]
    with torch.inference_mode():
        golden['features'] = {
            'frames': 24, 'input_seed': 5,
            'rows8': model.prepare_features(*inputs[:4]),
            'rows513': model.prepare_features(wide, *inputs[1:4]),
            'global': model.prepare_global_features(*inputs[4:7])}
        for key, rows in (('rows8', inputs[0]), ('rows513', wide)):
            mine = oracle.prepare_features(
                rows, *inputs[1:4], state['pitch_distribution'],
                state['pitch_embedding.weight'], state['ppg_threshold'])
            assert (mine - golden['features'][key]).abs().max() < 1e-6

    # spectrogram.from_audio (torch.stft inside the reference)
    gen = torch.Generator().manual_seed(7)
    one = torch.randn(1, 5120, generator=gen) * .1
    many = torch.randn(3, 1, 2560, generator=gen) * .1
    with torch.inference_mode():
        golden['spectrogram'] = {
            'one_input': one, 'many_input': many,
            'one': promonet.preprocess.spectrogram.from_audio(one),
            'many': promonet.preprocess.spectrogram.from_audio(many)}
    assert golden['spectrogram']['one'].shape == (513, 20)
    assert golden['spectrogram']['many'].shape == (3, 513, 10)
    for key in ('one', 'many'):
        mine = oracle.spectrogram(golden['spectrogram'][key + '_input'])
        assert (mine - golden['spectrogram'][key]).abs().max() < 1e-6
        dft = oracle.spectrogram_dft(golden['spectrogram'][key + '_input'])
        assert (dft - golden['spectrogram'][key].double().reshape(
            dft.shape)).abs().max() < 2e-5

    # promonet.edit: grid.sample is reference code; the grid constructor is the
    # stubbed third-party ppgs one (unpinned), so the grid is stored too
    gen = torch.Generator().manual_seed(8)
    frames = 37
    edit_inputs = oracle.synthetic_inputs(1, frames, seed=13)
    loud, pit, per, pg = (
        edit_inputs[0][0], edit_inputs[1], edit_inputs[2], edit_inputs[3][0])
    golden['edit'] = {'frames': frames, 'input_seed': 13, 'cases': []}
    for cents, ratio, db in (
        (None, 1.3, None), (200., None, None), (-700., .6, 3.5),
        (None, None, -2.)
    ):
        result = promonet.edit.from_features(
            loud.clone(), pit.clone(), per.clone(), pg.clone(), cents, ratio,
            db, return_grid=True)
        mine = oracle.edit_from_features(
            loud.clone(), pit.clone(), per.clone(), pg.clone(), cents, ratio,
            db, grid=result[4])
        for a, b in zip(result[:4], mine):
            assert a.shape == b.shape and (a - b).abs().max() < 1e-5
        golden['edit']['cases'].append({
            'pitch_shift_cents': cents, 'time_stretch_ratio': ratio,
            'loudness_scale_db': db, 'grid': result[4],
            'outputs': tuple(t.clone() for t in result[:4])})
    sequence = torch.randn(3, 21, generator=gen)
    grid = torch.rand(33, generator=gen) * 20.
    golden['edit']['sample'] = {
        'sequence': sequence, 'grid': grid,
        'linear': promonet.edit.grid.sample(sequence, grid),
        'nearest': promonet.edit.grid.sample(sequence, grid, 'nearest')}
    assert (oracle.grid_sample(sequence, grid) -
            golden['edit']['sample']['linear']).abs().max() < 1e-6

    # packed (nn~) interface: generator.py:255-422
    packed_inputs = oracle.synthetic_inputs(2, 16, seed=17)
    with torch.inference_mode():
        packed = model.pack_features(
            packed_inputs[0], packed_inputs[1][:, None],
            packed_inputs[2][:, None], *packed_inputs[3:])
        golden['packed'] = {
            'frames': 16, 'input_seed': 17, 'packed': packed,
            'audio': model.packed_inference(packed),
            'labels': len(model.labels())}
    assert packed.shape == (2, 53, 16)
    assert golden['packed']['audio'].shape == (2, 1, 16 * 256)

    # import-time constants the host mirror must reproduce
    golden['constants'] = {
        key: getattr(promonet, key) for key in (
            'NUM_FEATURES', 'GLOBAL_CHANNELS', 'NUM_SPEAKERS',
            'NUM_PREVIOUS_SAMPLES', 'SAMPLE_RATE', 'HOPSIZE', 'NUM_FFT',
            'WINDOW_SIZE', 'NUM_MELS', 'FMIN', 'FMAX', 'MIN_DB', 'REF_DB',
            'LOUDNESS_BANDS', 'PITCH_BINS', 'PITCH_EMBEDDING_SIZE',
            'PPG_CHANNELS', 'SPARSE_PPG_THRESHOLD', 'LRELU_SLOPE',
            'HIFIGAN_RESBLOCK_KERNEL_SIZES', 'HIFIGAN_RESBLOCK_DILATION_SIZES',
            'HIFIGAN_UPSAMPLE_INITIAL_SIZE', 'HIFIGAN_UPSAMPLE_KERNEL_SIZES',
            'HIFIGAN_UPSAMPLE_RATES', 'SPEAKER_CHANNELS')}
    golden['state_keys'] = {
        k: tuple(v.shape) for k, v in reference_state.items()}
    torch.save(golden, GOLDEN / 'generator_default.pt')


if __name__ == '__main__':
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for which in ('small', 'default', 'fargan', 'zero_shot',
                      'sparse_none', 'edit_voiced', 'layout'):
            subprocess.run(
                [sys.executable, __file__, which], check=True)
        for file in sorted(GOLDEN.iterdir()):
            print(file.name, file.stat().st_size, 'bytes')
