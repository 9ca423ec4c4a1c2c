"""SHA-256 digests of the 16-bit conv kernels' outputs, bit for bit.

The MFMA loop of the conv kernels (mma_taps, promonet_amd/csrc/pm_conv.h) may
change the ORDER IN WHICH IT ISSUES its loads and MFMAs, never the order in
which products are added into an accumulator: outputs stay bit-identical.
This script pins them. Run it on the GPU box on the commit BEFORE such a
change:

    python scripts/make_golden_mma_order.py --write

writes tests/golden/mma_order_digests.json, which tests/test_gpu_mma_order.py
compares against (it imports `unit_digests` / `forward_digests` from here).
A digest regenerated from the code under test pins nothing.

Cases, bf16 and f16 operands, seeded inputs (torch CPU generators):
  * pm_block_iteration_cl at C = 32, 64, 128, 256 x K = 3, 7, 11, dilations
    1, 3, 5;
  * pm_block_cl at the same shapes, three ways: the launcher's own choice on a
    short input, the walked variant forced (pm_debug_force) and the skewed
    walk forced (pm_debug_skew, scratch behind the workspace) - the form the
    batch-32 x 10 s step runs C = 128 k 11 in;
  * pm_mrf_cl at C = 32, 64, 128, 256 (all of K = 3, 7, 11 in one launch).
  A shape for which an entry has no kernel is pinned as the error it returns.
  * the full-size forward of bench.py's headline workload (batch 32 x 10 s,
    weights torch.manual_seed(0), inputs bench.synthetic_inputs seed 1234) in
    the 'bf16', 'f16' and 'checkpoint' operand modes.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'mma_order_digests.json'
# (the pm_debug_* hooks are off in a production process)
os.environ.setdefault('PROMONET_HIP_DEBUG', '1')
sys.path.insert(0, str(ROOT))

DTYPES = ('bf16', 'f16')
CHANNELS = (32, 64, 128, 256)
KERNEL_SIZES = (3, 7, 11)
DILATIONS = (1, 3, 5)
FORWARD_MODES = ('bf16', 'f16', 'checkpoint')


def sha256(tensor):
    """Digest of a tensor's bytes (contiguous, as laid out on the device)."""
    data = tensor.detach().contiguous().cpu().numpy().tobytes()
    return hashlib.sha256(data).hexdigest()


def to_cl(x):
    """(B, C, L) -> channels-last (B, L, C) (C is a multiple of 32 here)."""
    return x.permute(0, 2, 1).contiguous()


def attempt(call, out):
    """Digest of `out` after `call()`, or the library's refusal."""
    from promonet_amd import _lib
    try:
        call()
    except _lib.LibraryError as error:
        return f'error {error.code}'
    torch.cuda.synchronize()
    return sha256(out)


def conv_parameters(channels, kernel_size, count, gen, device):
    std = 1. / (channels * kernel_size) ** .5
    out = {'w1': [], 'b1': [], 'w2': [], 'b2': []}
    for _ in range(count):
        for which in (1, 2):
            w = torch.randn(channels, channels, kernel_size, generator=gen)
            b = torch.randn(channels, generator=gen) * .1
            out[f'w{which}'].append((w * std).to(device).contiguous())
            out[f'b{which}'].append(b.to(device).contiguous())
    return out


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def iteration_digests(device, dtype, channels, kernel_size):
    from promonet_amd import _lib
    library = _lib.lib()
    gen = torch.Generator().manual_seed(7000 + channels * 100 + kernel_size)
    size = library.pm_op_workspace_bytes(channels, channels, kernel_size)
    ws = torch.empty(size, dtype=torch.uint8, device=device)
    out = {}
    for dilation, length, mode in ((1, 301, 0), (3, 1257, 2), (5, 130, 1)):
        p = conv_parameters(channels, kernel_size, 1, gen, device)
        x_cl = to_cl(torch.randn(2, channels, length, generator=gen)).to(device)
        y = to_cl(torch.randn(2, channels, length, generator=gen)).to(device)
        out[f'd{dilation}_L{length}_m{mode}'] = attempt(
            lambda: _lib.check(library.pm_block_iteration_cl(
                _lib.DTYPES[dtype], _lib.ptr(x_cl), _lib.ptr(y),
                _lib.ptr(p['w1'][0]), _lib.ptr(p['b1'][0]),
                _lib.ptr(p['w2'][0]), _lib.ptr(p['b2'][0]), 2, length,
                channels, kernel_size, dilation, mode, 1 / 3, ws.data_ptr(),
                ws.numel(), _lib.stream())), y)
    return out


def block_digests(device, dtype, channels, kernel_size):
    from promonet_amd import _lib
    library = _lib.lib()
    gen = torch.Generator().manual_seed(8000 + channels * 100 + kernel_size)
    p = conv_parameters(channels, kernel_size, 3, gen, device)
    dil = (ctypes.c_int * 3)(*DILATIONS)
    weights = 3 * library.pm_op_workspace_bytes(
        channels, channels, kernel_size)
    scratch = library.pm_walk_scratch_bytes(2)
    ws = torch.empty(weights + scratch, dtype=torch.uint8, device=device)
    out = {}
    # (name, pm_debug_force segments, pm_debug_skew mode, workspace handed over)
    ways = (('plain', 0, -1, weights), ('walked', 2, -1, weights),
            ('skewed', 2, 1, weights + scratch))
    try:
        for length, mode in ((700, 0), (4645, 2), (61, 1)):
            x_cl = to_cl(
                torch.randn(2, channels, length, generator=gen)).to(device)
            prev = to_cl(
                torch.randn(2, channels, length, generator=gen)).to(device)
            for name, nseg, skew, size in ways:
                _lib.check(library.pm_debug_force(nseg, 0))
                _lib.check(library.pm_debug_skew(skew))
                y = prev.clone()
                out[f'{name}_L{length}_m{mode}'] = attempt(
                    lambda: _lib.check(library.pm_block_cl(
                        _lib.DTYPES[dtype], _lib.ptr(x_cl), _lib.ptr(y),
                        pointers(p['w1']), pointers(p['b1']),
                        pointers(p['w2']), pointers(p['b2']), dil, 3, 2,
                        length, channels, kernel_size, mode, 1 / 3,
                        ws.data_ptr(), size, _lib.stream())), y)
    finally:
        _lib.check(library.pm_debug_force(0, 0))
        _lib.check(library.pm_debug_skew(0))
    return out


def mrf_digests(device, dtype, channels):
    from promonet_amd import _lib
    library = _lib.lib()
    gen = torch.Generator().manual_seed(9000 + channels)
    p = {'w1': [], 'b1': [], 'w2': [], 'b2': []}
    for k in KERNEL_SIZES:
        block = conv_parameters(channels, k, 3, gen, device)
        for name in p:
            p[name] += block[name]
    dil = (ctypes.c_int * 3)(*DILATIONS)
    size = 9 * library.pm_op_workspace_bytes(channels, channels, 11)
    ws = torch.empty(size, dtype=torch.uint8, device=device)
    out = {}
    try:
        for nseg, length in ((0, 900), (0, 61), (2, 12000)):
            _lib.check(library.pm_debug_force(nseg, 0))
            x_cl = to_cl(
                torch.randn(2, channels, length, generator=gen)).to(device)
            y = torch.full_like(x_cl, 7.)
            out[f'nseg{nseg}_L{length}'] = attempt(
                lambda: _lib.check(library.pm_mrf_cl(
                    _lib.DTYPES[dtype], _lib.ptr(x_cl), _lib.ptr(y),
                    pointers(p['w1']), pointers(p['b1']), pointers(p['w2']),
                    pointers(p['b2']), dil, 3, 2, length, channels,
                    ws.data_ptr(), ws.numel(), _lib.stream())), y)
    finally:
        _lib.check(library.pm_debug_force(0, 0))
    return out


def unit_digests(device, dtype, channels, kernel_size):
    """{case: digest} of one (dtype, C, K) of the three unit entries."""
    out = {}
    for entry, digests in (
            ('iteration', iteration_digests(device, dtype, channels,
                                            kernel_size)),
            ('block', block_digests(device, dtype, channels, kernel_size))):
        out.update({f'{entry}_{k}': v for k, v in digests.items()})
    return out


def forward_digest(device, mode, batch=32, seconds=10.):
    """Digest of the audio of bench.py's headline step in operand mode `mode`
    (the second of two forwards; both must agree)."""
    import bench
    import promonet_amd
    frames = promonet_amd.convert.seconds_to_frames(seconds)
    promonet_amd.configure(COMPUTE_DTYPE=mode)
    try:
        torch.manual_seed(0)
        model = promonet_amd.model.Generator().to(device).eval()
        inputs = bench.synthetic_inputs(batch, frames, 1234, device)
        with torch.inference_mode():
            first = sha256(model(*inputs, None).float())
            second = sha256(model(*inputs, None).float())
        torch.cuda.synchronize()
    finally:
        promonet_amd.configure(
            COMPUTE_DTYPE=promonet_amd.config.DEFAULT_COMPUTE_DTYPE)
    assert first == second, 'the forward is not reproducible run to run'
    del model, inputs
    torch.cuda.empty_cache()
    return second


def all_digests(device):
    out = {'unit': {}, 'mrf': {}, 'forward': {}}
    for dtype in DTYPES:
        for channels in CHANNELS:
            out['mrf'][f'{dtype}_c{channels}'] = mrf_digests(
                device, dtype, channels)
            for kernel_size in KERNEL_SIZES:
                out['unit'][f'{dtype}_c{channels}_k{kernel_size}'] = \
                    unit_digests(device, dtype, channels, kernel_size)
    for mode in FORWARD_MODES:
        out['forward'][mode] = forward_digest(device, mode)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--write', action='store_true',
                        help=f'write {GOLDEN.relative_to(ROOT)}')
    parser.add_argument('--out', default=None,
                        help='write the digests to this file instead')
    args = parser.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    digests = all_digests(torch.device('cuda:0'))
    text = json.dumps(digests, indent=1, sort_keys=True) + '\n'
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    elif args.write:
        GOLDEN.write_text(text)
    else:
        sys.stdout.write(text)


if __name__ == '__main__':
    main()
