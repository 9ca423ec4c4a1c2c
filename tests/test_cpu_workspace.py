"""What every public sizing function of the C ABI answers, as a literal table.

A workspace layout is a data format: callers allocate `*_bytes` and the
launches place their buffers inside it. The numbers below were recorded from
the library as it was BEFORE each layout was stated once as a carve
(pm_host.h: PmCarve); the library under test has to give the same ones, slot
by conditional slot: with and without the gradient, 16-bit and fp32 operand
types, ragged and uniform, f16 and fp32 FARGAN storage, with and without the
walk's scratch. The engines' `create` calls are host-only, so this runs
without a GPU.

`PROMONET_HIP_LIB=<another build>/libpromonet_hip.so python
tests/test_cpu_workspace.py` prints the tables as that build answers them.
"""
import ctypes
import os
import sys
from pathlib import Path

import pytest

F32, F16, BF16, MIXED = 0, 1, 2, 16

# (entry, arguments, bytes)
TABLE = [
    ('pm_op_workspace_bytes', (113, 512, 7), 3997696),
    ('pm_op_workspace_bytes', (32, 32, 3), 45056),
    ('pm_op_workspace_bytes', (32, 32, 11), 110592),
    ('pm_op_workspace_bytes', (20, 20, 7), 77824),
    ('pm_op_workspace_bytes', (40, 32, 7), 135168),
    ('pm_op_workspace_bytes', (64, 32, 4), 86016),
    ('pm_op_workspace_bytes', (512, 256, 16), 16941056),
    ('pm_walk_scratch_bytes', (0,), 0),
    ('pm_walk_scratch_bytes', (2,), 67108864),
    ('pm_walk_scratch_bytes', (300,), 78643200),
    ('pm_stft_scratch_bytes', (2, 4096), 38912),
    ('pm_stft_scratch_bytes', (1, 256), 4096),
    ('pm_stft_scratch_bytes', (1, 255), 0),
    ('pm_stft_mel_scratch_bytes', (0,), 0),
    ('pm_stft_mel_scratch_bytes', (80,), 165376),
    ('pm_stft_mel_scratch_bytes', (128,), 264448),
    ('pm_stft_backward_scratch_bytes', (2, 4096), 217088),
    ('pm_stft_backward_scratch_bytes', (3, 1000), 76032),
    ('pm_stft_backward_scratch_bytes', (0, 4096), 0),
    ('pm_loudness_scratch_bytes', (2, 4096), 512),
    ('pm_loudness_scratch_bytes', (1, 256), 512),
    ('pm_loudness_scratch_bytes', (5, 100000), 1024),
    ('pm_loudness_scratch_bytes', (2, 100), 0),
    ('pm_limit_workspace_bytes', (0,), 0),
    ('pm_limit_workspace_bytes', (2,), 256),
    ('pm_limit_workspace_bytes', (100,), 1792),
    ('pm_viterbi_workspace', (2, 100, 360), 144128),
    ('pm_sc_forward_workspace_bytes', (3, 4096, 2560, 640, 1), 215552),
    ('pm_sc_forward_workspace_bytes', (3, 4096, 2560, 640, 0), 256),
    ('pm_sc_forward_workspace_bytes', (2, 8192, 1024, 256, 1), 271616),
    ('pm_sc_forward_workspace_bytes', (2, 8192, 1024, 256, 0), 512),
    ('pm_sc_forward_workspace_bytes', (3, 4096, 1000, 640, 1), 0),
    ('pm_sc_adjoint_workspace_bytes', (3, 4096, 2560, 640), 215040),
    ('pm_sc_adjoint_workspace_bytes', (2, 8192, 1024, 256), 270336),
    ('pm_signal_loss_workspace_bytes', (0,), 0),
    ('pm_signal_loss_workspace_bytes', (3,), 256),
    # (mode R, CMB, DB = 0, 1, 2; ...; win_length, pad, backward), recorded
    # before the transform's plan was stated once (pm_stockham.h): R's and
    # CMB's forward layouts are empty and answer 256; a refused size (T = pad)
    # answers 0
    ('pm_disc_spec_workspace_bytes', (0, 2, 4096, 1024, 120, 600, 452, 0),
     256),
    ('pm_disc_spec_workspace_bytes', (0, 2, 4096, 1024, 120, 600, 452, 1),
     557824),
    ('pm_disc_spec_workspace_bytes', (1, 2, 4096, 1024, 256, 1024, 384, 0),
     256),
    ('pm_disc_spec_workspace_bytes', (1, 2, 4096, 1024, 256, 1024, 384, 1),
     262400),
    ('pm_disc_spec_workspace_bytes', (2, 2, 1000, 64, 16, 64, 32, 0), 256),
    ('pm_disc_spec_workspace_bytes', (2, 2, 1000, 64, 16, 64, 32, 1), 66048),
    ('pm_disc_spec_workspace_bytes', (2, 40, 1000, 64, 16, 64, 32, 0), 512),
    ('pm_disc_spec_workspace_bytes', (2, 3, 3000, 2048, 512, 2048, 1024, 1),
     295680),
    ('pm_disc_spec_workspace_bytes', (0, 2, 231, 512, 50, 240, 231, 0), 0),
    ('pm_disc_spec_workspace_bytes', (0, 2, 231, 512, 50, 240, 231, 1), 0),
    ('pm_convnext_block_workspace_bytes', (F16, 512, 1536), 3160064),
    ('pm_convnext_block_workspace_bytes', (BF16, 512, 1024), 2111488),
    ('pm_convnext_block_workspace_bytes', (F32, 512, 1536), 6305792),
    ('pm_convnext_block_workspace_bytes', (7, 512, 1536), 0),
    ('pm_vocos_gemm_workspace_bytes', (F16, 7, 80, 512), 573440),
    ('pm_vocos_gemm_workspace_bytes', (F32, 7, 80, 512), 1146880),
    ('pm_vocos_gemm_workspace_bytes', (F16, 1, 512, 1026), 1179648),
    ('pm_vocos_gemm_workspace_bytes', (F32, 1, 512, 1026), 2359296),
    ('pm_vocos_gemm_workspace_bytes', (F16, 3, 512, 512), 0),
    ('pm_vocos_head_workspace_bytes', (F16, 2, 10), 1343744),
    ('pm_vocos_head_workspace_bytes', (F32, 2, 10), 2523392),
    ('pm_vocos_head_workspace_bytes', (BF16, 1, 1), 1188096),
    ('pm_vocos_head_workspace_bytes', (F16, 0, 10), 0),
    ('pm_istft_workspace_bytes', (2, 10), 81920),
    ('pm_istft_workspace_bytes', (0, 10), 0),
]

# elements of each tensor -> pm_multi_mean_workspace_bytes
MULTI_MEAN_TABLE = [
    ((1000, 70000, 5), 768),
    ((1,), 768),
    ((1 << 20,) * 40, 21760),
]

# (engine, entry, (batch, frames), bytes); a 'forced' engine is sized under
# pm_debug_force(2, 0), which adds the skewed walks' scratch to short calls
ENGINE_TABLE = [
    ('hifigan', 'pm_hifigan_workspace_bytes', (1, 16), 2107392),
    ('hifigan', 'pm_hifigan_workspace_bytes', (2, 24), 6320128),
    ('hifigan', 'pm_hifigan_workspace_bytes', (32, 861), 3692576768),
    ('hifigan forced', 'pm_hifigan_workspace_bytes', (1, 16), 69216256),
    ('hifigan small', 'pm_hifigan_workspace_bytes', (1, 16), 2105600),
    ('hifigan small forced', 'pm_hifigan_workspace_bytes', (1, 16), 69214464),
    ('vocos f16', 'pm_vocos_workspace_bytes', (2, 8), 135424),
    ('vocos f16', 'pm_vocos_ragged_workspace_bytes', (2, 8), 135936),
    ('vocos f16', 'pm_vocos_workspace_bytes', (32, 861), 225991936),
    ('vocos f16', 'pm_vocos_ragged_workspace_bytes', (32, 861), 226433024),
    ('vocos fp32', 'pm_vocos_workspace_bytes', (2, 5), 86272),
    ('vocos fp32', 'pm_vocos_ragged_workspace_bytes', (2, 5), 86784),
    ('fargan f16', 'pm_fargan_workspace_bytes', (2, 2), 6820096),
    ('fargan fp32', 'pm_fargan_workspace_bytes', (2, 2), 6828288),
    ('fargan mixed', 'pm_fargan_workspace_bytes', (2, 2), 6828288),
    ('fargan f16', 'pm_fargan_workspace_bytes', (32, 100), 8456448),
    ('fargan fp32', 'pm_fargan_workspace_bytes', (32, 100), 15010048),
]


def library():
    from promonet_amd import _lib
    return _lib


def hifigan_config(initial_channels):
    _lib = library()
    config = _lib.HifiganConfig()
    config.num_features, config.global_channels = 113, 258
    config.initial_channels, config.num_stages = initial_channels, 4
    for i, (r, k) in enumerate(zip((8, 8, 2, 2), (16, 16, 4, 4))):
        config.upsample_rates[i], config.upsample_kernel_sizes[i] = r, k
    config.num_resblocks, config.num_dilations = 3, 3
    for j, k in enumerate((3, 7, 11)):
        config.resblock_kernel_sizes[j] = k
        for n, d in enumerate((1, 3, 5)):
            config.resblock_dilations[j][n] = d
    config.compute_dtype = F16
    return config


def create(engine):
    """-> (handle, destroy) of the engine a row of ENGINE_TABLE names"""
    lib = library().lib()
    handle = ctypes.c_void_p()
    kind, *variant = engine.split()
    if kind == 'hifigan':
        config = hifigan_config(64 if 'small' in variant else 512)
        code = lib.pm_hifigan_create(
            ctypes.byref(config), ctypes.byref(handle))
    elif kind == 'vocos':
        dtype = {'f16': F16, 'fp32': F32}[variant[0]]
        code = lib.pm_vocos_create(
            80, 256, 512, 1536, 1, 1024, 256, dtype, ctypes.byref(handle))
    else:
        dtype = {'f16': F16, 'fp32': F32, 'mixed': MIXED}[variant[0]]
        code = lib.pm_fargan_create(113, 258, dtype, ctypes.byref(handle))
    assert code == 0, lib.pm_last_error()
    return handle, getattr(lib, f'pm_{kind}_destroy')


def engine_bytes(engine, entry, shape):
    lib = library().lib()
    handle, destroy = create(engine)
    try:
        if 'forced' in engine:
            assert lib.pm_debug_force(2, 0) == 0, lib.pm_last_error()
        return getattr(lib, entry)(handle, *shape)
    finally:
        if 'forced' in engine:
            assert lib.pm_debug_force(0, 0) == 0
        destroy(handle)


def multi_mean_bytes(numel):
    array = (ctypes.c_longlong * len(numel))(*numel)
    return library().lib().pm_multi_mean_workspace_bytes(array, len(numel))


@pytest.mark.parametrize(
    'entry,arguments,want', TABLE,
    ids=[f'{entry}{arguments}' for entry, arguments, _ in TABLE])
def test_cpu_sizing_table(entry, arguments, want):
    assert getattr(library().lib(), entry)(*arguments) == want


@pytest.mark.parametrize('numel,want', MULTI_MEAN_TABLE,
                         ids=[str(len(n)) for n, _ in MULTI_MEAN_TABLE])
def test_cpu_multi_mean_sizing_table(numel, want):
    assert multi_mean_bytes(numel) == want


@pytest.mark.parametrize(
    'engine,entry,shape,want', ENGINE_TABLE,
    ids=[f'{engine}:{entry}{shape}' for engine, entry, shape, _ in ENGINE_TABLE])
def test_cpu_engine_sizing_table(engine, entry, shape, want):
    assert engine_bytes(engine, entry, shape) == want
    # (a null handle and an empty call size to nothing)
    assert getattr(library().lib(), entry)(None, *shape) == 0
    assert engine_bytes(engine, entry, (0, shape[1])) == 0


if __name__ == '__main__':
    os.environ.setdefault('PROMONET_HIP_DEBUG', '1')
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    for entry, arguments, _ in TABLE:
        print(f'    ({entry!r}, {arguments}, '
              f'{getattr(library().lib(), entry)(*arguments)}),')
    for numel, _ in MULTI_MEAN_TABLE:
        print(f'    ({len(numel)} tensors, {multi_mean_bytes(numel)}),')
    for engine, entry, shape, _ in ENGINE_TABLE:
        print(f'    ({engine!r}, {entry!r}, {shape}, '
              f'{engine_bytes(engine, entry, shape)}),')
