"""The last two kernels of the Vocos uniform path, vocos_istft_frame_kernel
and vocos_ola_kernel (pm_vocos.h), per bin and exactly, against the float64
oracle of tests/vocos_head_oracle.py. The ragged head is held equal to the
uniform one by tests/test_gpu_vocos_ragged.py, so this anchors both.

  per bin  one bin alone in every fourth frame, through pm_istft (the
           spectrum entry) and through pm_vocos_head (the logits entry:
           expf, the clip at 100, sincosf) in every operand type: the error
           of each bin over its own samples, relative to its own RMS, within
           4 x the error of the reference's own fp32 arithmetic
  exact    bins 0 and 512 on a grid where fp32 is exact but for one correctly
           rounded division: torch.equal, at 1, 2, 3, 4, 5 and 9 frames; every
           sample written, none past the end
  modes    one-hot activations make the logits exact in fp32, f16 and bf16:
           the three give the same audio bit for bit

tests/test_cpu_vocos_head.py shows that these comparisons reject every
planted defect of the oracle.

Measured on an MI355X (printed by the tests): worst
per-bin figure of the spectrum entry 9.336e-07 (bin 285) where the
reference's fp32 arithmetic has 1.043e-06 (gate 4.172e-06); of the logits
entry 9.101e-07 (bin 282; 8.740e-07 in the low set, bin 503), the same in
fp32, f16 and bf16, where it has 1.029e-06 (gate 4.116e-06); the frames at
log-magnitude 4.5, 4.625 and 5 within 7.644e-07. The exact table is equal at
every frame count.
"""
import pytest
import torch

from promonet_amd import _lib

import vocos_head_oracle as oracle

pytestmark = pytest.mark.gpu

DTYPES = ('fp32', 'f16', 'bf16')


def run_istft(spec, window, guard=0):
    """pm_istft into a buffer of NaN with `guard` more floats behind it"""
    batch, _, frames = spec.shape
    lib = _lib.lib()
    pairs = torch.view_as_real(spec.to(torch.complex64)).contiguous().cuda()
    window = window.float().contiguous().cuda()
    size = batch * frames * 256
    out = torch.full((size + guard,), float('nan'), device='cuda')
    ws = torch.empty(lib.pm_istft_workspace_bytes(batch, frames),
                     dtype=torch.uint8, device='cuda')
    _lib.check(lib.pm_istft(
        _lib.ptr(pairs), _lib.ptr(window), _lib.ptr(out), batch, frames,
        ws.data_ptr(), ws.numel(), _lib.stream()))
    out = out.cpu()
    return out[:size].view(batch, frames * 256), out[size:]


def test_each_bin_alone(device):
    spec, window, live = oracle.per_bin_table()
    got, _ = run_istft(spec, window)
    want = oracle.per_bin_oracle()
    assert got.shape == want.shape
    worst, where = oracle.figure(got, want, live)
    print(f'spectrum entry, worst bin: {worst:.3e} at bin {where[2]} (row '
          f'{where[0]}, frame {where[1]}); fp32 reference '
          f'{oracle.PER_BIN_FP32_FIGURE:.3e}, gate {oracle.PER_BIN_GATE:.3e}')
    assert worst < oracle.PER_BIN_GATE, (worst, where)
    # past the last live frame only zero frames contribute
    assert (got[:, oracle.span(4 * 512, spec.shape[2])[1]:] == 0).all()


@pytest.mark.parametrize('frames', oracle.EXACT_FRAMES)
def test_dc_and_nyquist_are_exact(device, frames):
    """oracle.exact_table has the derivation: only the last division rounds,
    and it rounds correctly, so the fp32 result is unique"""
    spec, window = oracle.exact_table(frames)
    got, guard = run_istft(spec, window, guard=1024)
    want = oracle.exact_oracle(frames)
    assert not got.isnan().any()            # every sample is written
    assert guard.isnan().all()              # and none behind the last
    assert torch.equal(got, want), (got != want).nonzero()[:8]


_audio = {}


def run_head(which, dtype):
    """pm_vocos_head on a head table, once: (2, 256 T) on the CPU"""
    if (which, dtype) not in _audio:
        x, weight, window, _ = oracle.head_table(which)
        batch, frames, _ = x.shape
        lib = _lib.lib()
        code = _lib.DTYPES[dtype]
        tensors = [t.contiguous().cuda()
                   for t in (x, weight, torch.zeros(1026), window)]
        out = torch.full((batch, frames * 256), float('nan'), device='cuda')
        ws = torch.empty(
            lib.pm_vocos_head_workspace_bytes(code, batch, frames),
            dtype=torch.uint8, device='cuda')
        _lib.check(lib.pm_vocos_head(
            code, *[_lib.ptr(t) for t in tensors], _lib.ptr(out), batch,
            frames, ws.data_ptr(), ws.numel(), _lib.stream()))
        _audio[which, dtype] = out.cpu()
    return _audio[which, dtype]


@pytest.mark.parametrize('dtype', DTYPES)
def test_head_each_bin_alone(device, dtype):
    for which in oracle.HEAD_SETS:
        live = oracle.head_table(which)[3]
        got = run_head(which, dtype)
        want = oracle.head_oracle(which)
        assert got.shape == want.shape
        worst, where = oracle.figure(got, want, live)
        print(f'logits entry {dtype} {which}, worst bin: {worst:.3e} at bin '
              f'{where[3]} (row {where[0]}, frame {where[1]}, log-magnitude '
              f'{where[4]}); fp32 reference {oracle.HEAD_FP32_FIGURE:.3e}, '
              f'gate {oracle.HEAD_GATE:.3e}')
        assert worst < oracle.HEAD_GATE, (which, worst, where)
        # expf(-128) = 0: where only all-silent frames reach, exact zeros
        assert (got[:, oracle.head_silence(which):] == 0).all()


def test_head_modes_agree_bit_for_bit(device):
    """The logits are exact in every operand type, so this is the handoff
    from the matrix product (ldo = 1026, phase at column 513 + k) into the
    transform with no tolerance"""
    for which in oracle.HEAD_SETS:
        single = run_head(which, 'fp32')
        assert not single.isnan().any() and single.abs().max() > 0
        for dtype in ('f16', 'bf16'):
            assert torch.equal(run_head(which, dtype), single), (which, dtype)


def test_clip_sides(device):
    """e^4.5 = 90 passes the clip, e^4.625 = 102 and e^5 = 148 come out as
    100. A clip elsewhere or on the other side moves these frames by 0.02 of
    their RMS at the least (test_cpu_vocos_head.py), the gate is 4e-6."""
    for which in oracle.HEAD_SETS:
        got = run_head(which, 'fp32')
        want = oracle.head_oracle(which)
        for value in oracle.CLIP_SIDES:
            live = [entry for entry in oracle.head_table(which)[3]
                    if entry[4] == value]
            assert len(live) >= 10
            worst, where = oracle.figure(got, want, live)
            print(f'{which}, log-magnitude {value}: {worst:.3e}')
            assert worst < oracle.HEAD_GATE, (which, value, worst, where)
