"""The 16-bit conv kernels' outputs, bit for bit, against SHA-256 digests
taken before the MFMA loop's issue order was reworked
(tests/golden/mma_order_digests.json, written by
scripts/make_golden_mma_order.py on the parent commit): the loop may change
the order in which it ISSUES loads and MFMAs, never the order in which products
are added into an accumulator. The cases and their seeded inputs are that
script's; there is no tolerance."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads(
    (ROOT / 'tests' / 'golden' / 'mma_order_digests.json').read_text())


def cases():
    spec = importlib.util.spec_from_file_location(
        'make_golden_mma_order', ROOT / 'scripts' / 'make_golden_mma_order.py')
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def compare(got, want, what):
    assert sorted(got) == sorted(want), what
    different = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    print(f'{what}: {len(want) - len(different)} of {len(want)} digests equal')
    assert not different, (what, different)


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('channels', [32, 64, 128, 256])
@pytest.mark.parametrize('kernel_size', [3, 7, 11])
def test_block_entries_bit_for_bit(device, dtype, channels, kernel_size):
    """pm_block_iteration_cl and pm_block_cl (the launcher's choice, the
    walked and the skewed whole Block)."""
    key = f'{dtype}_c{channels}_k{kernel_size}'
    compare(cases().unit_digests(device, dtype, channels, kernel_size),
            GOLDEN['unit'][key], key)


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('channels', [32, 64, 128, 256])
def test_mrf_entry_bit_for_bit(device, dtype, channels):
    """pm_mrf_cl: Blocks k 3, 7, 11 of one stage in one launch."""
    key = f'{dtype}_c{channels}'
    compare(cases().mrf_digests(device, dtype, channels),
            GOLDEN['mrf'][key], key)


@pytest.mark.parametrize('mode', ['bf16', 'f16', 'checkpoint'])
def test_full_size_forward_bit_for_bit(device, mode):
    """The batch-32 x 10 s step of bench.py, whole generator."""
    got = cases().forward_digest(device, mode)
    print(f'forward {mode}: {got}')
    assert got == GOLDEN['forward'][mode], mode
