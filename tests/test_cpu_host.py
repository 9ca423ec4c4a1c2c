"""CPU: host logic of the drop-in package and the C-ABI surface (no compute
calls - there is no GPU here)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import promonet_amd
from promonet_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    declared = set(re.findall(r'\b(pm_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 25
    library = _lib.lib()
    for name in declared:
        assert hasattr(library, name), name
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert library.pm_version() >= 100


def make_config(**overrides):
    config = _lib.HifiganConfig()
    config.num_features, config.global_channels = 113, 258
    config.initial_channels, config.num_stages = 512, 4
    for i, (r, k) in enumerate(zip((8, 8, 2, 2), (16, 16, 4, 4))):
        config.upsample_rates[i], config.upsample_kernel_sizes[i] = r, k
    config.num_resblocks, config.num_dilations = 3, 3
    for j, k in enumerate((3, 7, 11)):
        config.resblock_kernel_sizes[j] = k
        for n, d in enumerate((1, 3, 5)):
            config.resblock_dilations[j][n] = d
    config.compute_dtype = _lib.PM_F16
    for key, value in overrides.items():
        setattr(config, key, value)
    return config


def test_engine_create_validates_configuration():
    """pm_hifigan_create is host-only: error codes + messages, no exceptions
    across the boundary."""
    library = _lib.lib()
    handle = ctypes.c_void_p()
    assert library.pm_hifigan_create(
        ctypes.byref(make_config()), ctypes.byref(handle)) == 0
    assert library.pm_hifigan_hopsize(handle) == 256
    assert library.pm_hifigan_features_cl_channels(handle) == 128
    size = library.pm_hifigan_workspace_bytes(handle, 32, 861)
    # 4 rotating fp32 activation buffers of 32 x 861 x 8192 floats + features
    # + the scratch of the skewed whole-Block walk (256 KiB per workgroup,
    # max(batch, CUs) workgroups: 64 MiB)
    buffers = 4 * 32 * 861 * 8192 * 4
    assert buffers + 2 ** 26 <= size < buffers + 2 ** 26 + 2 ** 25
    assert library.pm_walk_scratch_bytes(32) == 2 ** 26
    # (a single 2 s utterance never takes the skewed walk: no scratch)
    assert library.pm_hifigan_workspace_bytes(handle, 1, 172) < 2 ** 26
    assert library.pm_walk_scratch_bytes(0) == 0
    # forward before finalize / with null pointers is refused, not a crash
    assert library.pm_hifigan_forward(
        handle, None, None, 1, None, 1, 8, None, 0, None) == -1
    assert library.pm_hifigan_finalize(handle, None) == -2
    assert b'missing tensor' in library.pm_last_error()
    assert library.pm_hifigan_destroy(handle) == 0

    bad = make_config()
    bad.resblock_kernel_sizes[1] = 5
    assert library.pm_hifigan_create(
        ctypes.byref(bad), ctypes.byref(handle)) == -1
    assert b'kernel size 5' in library.pm_last_error()
    bad = make_config()
    bad.upsample_kernel_sizes[0] = 15
    assert library.pm_hifigan_create(
        ctypes.byref(bad), ctypes.byref(handle)) == -1
    bad = make_config(compute_dtype=7)
    assert library.pm_hifigan_create(
        ctypes.byref(bad), ctypes.byref(handle)) == -1
    # the stage types of the 'checkpoint' schedule (promonet_hip.h: PM_F16A2 =
    # activations split, PM_F16UX = f16 Blocks behind a fully split upsampler)
    # are accepted per engine and per stage; one past them is not
    from promonet_amd.model.hifigan import checkpoint_schedule
    assert checkpoint_schedule(4) == ['f16', 'f16', 'f16ux', 'f16a2']
    assert checkpoint_schedule(2) == ['f16ux', 'f16a2']
    assert checkpoint_schedule(1) == ['f16a2']
    assert (_lib.PM_F16A2, _lib.PM_F16UX) == (4, 5)
    good = make_config(compute_dtype=_lib.PM_F16)
    good.stage_compute_dtype[2] = 1 + _lib.PM_F16UX
    good.stage_compute_dtype[3] = 1 + _lib.PM_F16A2
    assert library.pm_hifigan_create(
        ctypes.byref(good), ctypes.byref(handle)) == 0
    assert library.pm_hifigan_destroy(handle) == 0
    bad = make_config()
    bad.stage_compute_dtype[3] = 2 + _lib.PM_F16UX
    assert library.pm_hifigan_create(
        ctypes.byref(bad), ctypes.byref(handle)) == -1
    assert b'stage_compute_dtype[3]' in library.pm_last_error()
    bad = make_config()
    bad.resblock_dilations[0][2] = 9
    assert library.pm_hifigan_create(
        ctypes.byref(bad), ctypes.byref(handle)) == -1
    with pytest.raises(RuntimeError, match='libpromonet_hip error -1'):
        _lib.check(-1)


def test_constants_match_reference(golden_default):
    for key, value in golden_default['constants'].items():
        assert getattr(promonet_amd, key) == value, key


def test_state_dict_is_the_reference_contract(golden_default):
    """Same keys and shapes as the reference Generator.state_dict()."""
    model = promonet_amd.model.Generator()
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert mine == golden_default['state_keys']
    assert sum(p.numel() for p in model.parameters()) == 14_230_784
    assert torch.equal(
        model.pitch_distribution, golden_default['pitch_distribution'])
    # weight-normed init: g == ||v|| so that w == v (hifigan.py:220-223)
    state = model.state_dict()
    v = state['model.model.1.model.2.model.2.convs1.1.weight_v']
    g = state['model.model.1.model.2.model.2.convs1.1.weight_g']
    assert torch.allclose(g, torch.linalg.vector_norm(v, dim=(1, 2), keepdim=True))
    assert abs(v.std().item() - .01) < 1e-3


def test_no_cpu_fallback():
    import restatement as oracle
    model = promonet_amd.model.Generator()
    inputs = oracle.synthetic_inputs(1, 8)
    with pytest.raises(RuntimeError, match='AMD GPU'):
        model(*inputs, None)
    with pytest.raises(RuntimeError, match='AMD GPU'):
        promonet_amd.synthesize.from_features(*inputs[:4])
    with pytest.raises(RuntimeError, match='AMD GPU'):
        promonet_amd.preprocess.spectrogram.from_audio(torch.zeros(1, 4096))
    with pytest.raises(RuntimeError, match='AMD GPU'):
        promonet_amd.preprocess.from_audio(torch.zeros(1, 4096))


def test_product_never_imports_the_oracle():
    for file in (ROOT / 'promonet_amd').rglob('*.py'):
        text = file.read_text()
        assert 'restatement' not in text and 'import oracle' not in text, file


def test_convert():
    assert promonet_amd.convert.seconds_to_frames(2) == 172
    assert promonet_amd.convert.seconds_to_frames(5) == 430
    assert promonet_amd.convert.seconds_to_frames(10) == 861
    assert promonet_amd.convert.samples_to_frames(220416) == 861
    assert promonet_amd.convert.frames_to_samples(861) == 220416
    assert promonet_amd.convert.db_to_ratio(10.) == 2.
    assert abs(promonet_amd.convert.ratio_to_db(2.) - 10.) < 1e-12
    bins = promonet_amd.convert.hz_to_bins(torch.tensor([1., 56., 9999.]))
    assert bins.tolist() == [0, 1, 255]


def test_configure_rederives_static_constants():
    try:
        promonet_amd.configure(LOUDNESS_BANDS=4)
        assert promonet_amd.NUM_FEATURES == 109
    finally:
        promonet_amd.configure(LOUDNESS_BANDS=8)
    assert promonet_amd.NUM_FEATURES == 113
    with pytest.raises(ValueError):
        promonet_amd.configure(NOT_A_PARAMETER=1)


def test_checkpoint_round_trip(tmp_path):
    """torchutil-style checkpoint ({'model': state_dict}) and a bare state
    dict both load; keys are the reference's."""
    model = promonet_amd.model.Generator()
    file = tmp_path / 'generator-00000001.pt'
    torch.save({'model': model.state_dict(), 'step': 1}, file)
    other = promonet_amd.model.Generator()
    promonet_amd.synthesize.load_checkpoint(file, other)
    for (ka, va), (kb, vb) in zip(
            model.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    torch.save(model.state_dict(), file)
    promonet_amd.synthesize.load_checkpoint(file, other)


def test_loudness_host_helpers():
    import restatement as oracle
    gen = torch.Generator().manual_seed(0)
    loudness = torch.rand(2, 513, 7, generator=gen) * 80 - 100
    got = promonet_amd.preprocess.loudness.band_average(loudness, 8)
    assert torch.equal(got, oracle.band_average(loudness, 8))
    assert torch.equal(
        promonet_amd.preprocess.loudness.normalize(got), oracle.normalize(got))
    import numpy as np
    assert np.array_equal(
        promonet_amd.preprocess.loudness.perceptual_weights(),
        oracle.perceptual_weights())
    assert torch.allclose(
        promonet_amd.preprocess.spectrogram.mel_basis(), oracle.mel_basis(),
        atol=1e-8)


def test_fargan_state_dict_contract(golden_fargan):
    try:
        promonet_amd.configure(MODEL='fargan')
        assert promonet_amd.NUM_PREVIOUS_SAMPLES == \
            golden_fargan['num_previous_samples'] == 512
        model = promonet_amd.model.Generator()
    finally:
        promonet_amd.configure(MODEL='hifigan')
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert mine == golden_fargan['state_keys']
    assert sum(p.numel() for p in model.model.parameters()) == 2_714_642 \
        or sum(p.numel() for p in model.parameters()) > 2_700_000
    # orthogonal init (fargan.py:418-424)
    w = model.model.state_dict()['conditioning_network.0.weight']
    assert torch.allclose(w @ w.T, torch.eye(371), atol=1e-4)
    assert promonet_amd.NUM_PREVIOUS_SAMPLES == 1


def test_fargan_engine_validation():
    import ctypes
    library = _lib.lib()
    handle = ctypes.c_void_p()
    assert library.pm_fargan_create(113, 258, _lib.PM_F32,
                                    ctypes.byref(handle)) == 0
    assert library.pm_fargan_finalize(handle, None) == -2
    assert b'conditioning_network.0' in library.pm_last_error()
    assert library.pm_fargan_destroy(handle) == 0
    assert library.pm_fargan_create(80, 258, _lib.PM_F32,
                                    ctypes.byref(handle)) == -1
    assert library.pm_fargan_create(113, 258, _lib.PM_BF16,
                                    ctypes.byref(handle)) == -1
    # the mixed weight storage (GRU cells / GLU gates f16, the rest fp32):
    # the Python table carries the header's constant
    header = (ROOT / 'include' / 'promonet_hip.h').read_text()
    mixed = int(re.search(r'#define PM_FARGAN_MIXED (\d+)', header).group(1))
    assert _lib.DTYPES['mixed'] == mixed
    assert library.pm_fargan_create(113, 258, mixed,
                                    ctypes.byref(handle)) == 0
    assert library.pm_fargan_destroy(handle) == 0
    # ... and is not an MFMA operand type of the HiFi-GAN engine
    assert mixed not in (_lib.PM_F32, _lib.PM_F16, _lib.PM_BF16, _lib.PM_F16X3)


def reference_stand_in():
    """A package object of the reference's shape, rebuilt from the layout
    oracle/make_golden.py recorded from the real one
    (tests/golden/reference_layout.json): its constants, and a placeholder
    for every module, class and function the patch replaces."""
    import json
    import types
    layout = json.loads(
        (ROOT / 'tests' / 'golden' / 'reference_layout.json').read_text())
    promonet = types.ModuleType('promonet')
    promonet.__dict__.update(layout['constants'])
    for name in layout['opaque_constants']:
        setattr(promonet, name, object())
    for path, kind in sorted(layout['attributes'].items()):
        *parents, leaf = path.split('.')
        owner = promonet
        for part in parents:
            if not hasattr(owner, part):
                setattr(owner, part, types.ModuleType(part))
            owner = getattr(owner, part)
        if not hasattr(owner, leaf):
            setattr(owner, leaf, types.ModuleType(leaf) if kind == 'module'
                    else type(leaf, (), {}) if kind == 'class'
                    else lambda *args, **kwargs: None)
    return promonet, layout


def test_patch_swaps_into_the_real_reference():
    """The literal drop-in of INTEGRATION.md section 1, on a stand-in of the
    reference package recorded from the real one: every constant agrees (the
    patch reconfigures nothing), and everything it swaps in is an attribute
    the reference has."""
    promonet, layout = reference_stand_in()
    before = {n: getattr(promonet_amd, n) for n in dir(promonet_amd.config)
              if n.isupper()}
    modules = {
        path: set(vars(module)) for path, module in (
            ('', promonet), ('model', promonet.model),
            ('synthesize', promonet.synthesize),
            ('synthesize.core', promonet.synthesize.core),
            ('preprocess.spectrogram', promonet.preprocess.spectrogram),
            ('preprocess.loudness', promonet.preprocess.loudness))}
    original = promonet.synthesize.from_features
    promonet_amd.patch(promonet)
    try:
        assert before == {n: getattr(promonet_amd, n) for n in before}
        for path, names in modules.items():
            module = promonet
            for part in filter(None, path.split('.')):
                module = getattr(module, part)
            assert set(vars(module)) == names, path
        assert promonet.model.Generator is promonet_amd.model.Generator
        assert promonet.model.HiFiGAN is promonet_amd.model.HiFiGAN
        assert promonet.synthesize.from_features is \
            promonet_amd.synthesize.from_features
        assert promonet.synthesize.core.generate is \
            promonet_amd.synthesize.generate
        assert promonet.preprocess.spectrogram.from_audio is \
            promonet_amd.preprocess.spectrogram.from_audio
        # same constructor contract: no arguments, reference state-dict keys
        model = promonet.model.Generator()
        assert len(model.state_dict()) == 238 == \
            layout['generator_state_dict_entries']
        assert promonet_amd.NUM_FEATURES == promonet.NUM_FEATURES
    finally:
        promonet.synthesize.from_features = original


def test_no_kernel_spills():
    """Every kernel of the shipped library fits its registers: no VGPR spill,
    no scratch memory (scripts/check_spills.py reads the kernel metadata of
    the objects `make` built; VERDICT r01 found two spilling hot kernels)."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    objects = sorted((root / 'build' / 'obj').glob('pm_*.o'))
    if len(objects) < 4:
        pytest.skip('objects not built here (make)')
    done = subprocess.run(
        [sys.executable, str(root / 'scripts' / 'check_spills.py')] +
        [str(o) for o in objects],
        capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]


def test_makefile_objects_are_the_hip_sources():
    """The Makefile is the one place that lists the library's objects, and it
    lists every promonet_amd/csrc/*.hip (the variant scripts take the list
    from it: `make -s objs`)."""
    import subprocess
    done = subprocess.run(['make', '-s', 'objs'], cwd=ROOT, check=True,
                          capture_output=True, text=True)
    listed = sorted(Path(o).stem for o in done.stdout.split())
    sources = sorted(
        p.stem for p in (ROOT / 'promonet_amd' / 'csrc').glob('*.hip'))
    assert len(sources) >= 16
    assert listed == sources


def test_library_exports_exactly_the_signatures():
    """The pm_* symbols the built library defines are the entries of
    _lib.SIGNATURES, no more and no fewer: _lib.lib() resolves every entry, so
    a library linked from a stale object list does not load at all."""
    import subprocess
    if not _lib.LIB_PATH.exists():
        pytest.skip('library not built here (make)')
    done = subprocess.run(['nm', '-D', '--defined-only', str(_lib.LIB_PATH)],
                          check=True, capture_output=True, text=True)
    exported = {line.split()[-1] for line in done.stdout.splitlines()
                if line.strip()}
    exported = {name for name in exported if name.startswith('pm_')}
    assert exported == set(_lib.SIGNATURES), exported ^ set(_lib.SIGNATURES)


def test_debug_hooks_are_off_in_a_production_process():
    """pm_debug_force / pm_debug_skew change launch geometry: they answer
    PM_ESTATE unless the process opted in with PROMONET_HIP_DEBUG=1 (this
    test session does, tests/conftest.py), and their state is per host
    thread."""
    import os
    import subprocess
    import sys
    import threading
    code = (
        'from promonet_amd import _lib\n'
        'lib = _lib.lib()\n'
        'print(lib.pm_debug_force(2, 0), lib.pm_debug_skew(1), '
        'lib.pm_last_error().decode())\n')
    env = {k: v for k, v in os.environ.items() if k != 'PROMONET_HIP_DEBUG'}
    env['PYTHONPATH'] = str(ROOT)
    out = subprocess.run(
        [sys.executable, '-c', code], env=env, capture_output=True, text=True,
        timeout=300)
    assert out.returncode == 0, out.stderr
    first, second, message = out.stdout.strip().split(' ', 2)
    assert int(first) == int(second) == _lib.PM_ESTATE
    assert 'PROMONET_HIP_DEBUG' in message
    # opted in: accepted, and another thread still sees the defaults - its
    # workspace query (which depends on the forced walk) is unchanged
    library = _lib.lib()
    handle = ctypes.c_void_p()
    assert library.pm_hifigan_create(
        ctypes.byref(make_config()), ctypes.byref(handle)) == 0
    plain = library.pm_hifigan_workspace_bytes(handle, 1, 16)
    assert library.pm_debug_force(2, 0) == 0
    try:
        forced = library.pm_hifigan_workspace_bytes(handle, 1, 16)
        seen = []
        worker = threading.Thread(target=lambda: seen.append(
            library.pm_hifigan_workspace_bytes(handle, 1, 16)))
        worker.start()
        worker.join()
        assert forced > plain and seen == [plain]
    finally:
        assert library.pm_debug_force(0, 0) == 0
        library.pm_hifigan_destroy(handle)


def test_last_launch_hook_before_any_launch():
    """pm_debug_last_launch reports what a launch recorded on the calling
    host thread: PM_ESTATE where the hooks are off, and - opted in - on a
    thread that has launched no whole-Block or whole-MRF kernel yet."""
    import os
    import subprocess
    import sys
    import threading
    code = (
        'import ctypes\n'
        'from promonet_amd import _lib\n'
        'lib = _lib.lib()\n'
        'v = [ctypes.c_int(-7) for _ in range(4)]\n'
        'print(lib.pm_debug_last_launch(*[ctypes.byref(i) for i in v]), '
        '[i.value for i in v], lib.pm_last_error().decode())\n')
    env = {k: v for k, v in os.environ.items() if k != 'PROMONET_HIP_DEBUG'}
    env['PYTHONPATH'] = str(ROOT)
    out = subprocess.run(
        [sys.executable, '-c', code], env=env, capture_output=True, text=True,
        timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith(f'{_lib.PM_ESTATE} [-7, -7, -7, -7] ')
    assert 'PROMONET_HIP_DEBUG' in out.stdout
    library = _lib.lib()
    seen = []

    def fresh_thread():
        values = [ctypes.c_int(-7) for _ in range(4)]
        seen.append((library.pm_debug_last_launch(
            *[ctypes.byref(v) for v in values]), [v.value for v in values],
            library.pm_last_error().decode()))

    worker = threading.Thread(target=fresh_thread)
    worker.start()
    worker.join()
    code, values, message = seen[0]
    assert code == _lib.PM_ESTATE and values == [-7] * 4
    assert 'launch' in message and 'PROMONET_HIP_DEBUG' not in message
    values = [ctypes.c_int() for _ in range(3)]
    assert library.pm_debug_last_launch(
        *[ctypes.byref(v) for v in values], None) == _lib.PM_EINVAL
