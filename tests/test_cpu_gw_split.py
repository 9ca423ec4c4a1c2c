"""The partials of the pixel-GEMM gW kernels without a GPU: the workspace
queries of the period, generator and strided frequency layers are pure host
code, and all three count their partials by one formula (pm_chunk_split,
pm_host.h). `split` restates it once; the constants of each family are read
from its header through its oracle.

A partial is one workgroup's gW | gb of a tile. K = output pixels runs in
chunks of PIX pixels; a tile's chunks are shared among
    min(ceil(chunks / MIN_CHUNKS), max(WORKGROUPS / tiles, 1))
partials at the most, `each` = ceil(chunks / that) chunks a partial, so
ceil(chunks / each) partials are written.
"""
import pytest

from promonet_amd import _lib

import fdisc_strided_oracle
import gconv_oracle
import pconv_oracle


def split(pixels, pixels_per_chunk, tiles, workgroups, min_chunks):
    """(partials, chunks of each, chunks)"""
    chunks = -(-pixels // pixels_per_chunk)
    room = max(workgroups // tiles, 1)
    want = min(-(-chunks // min_chunks), room)
    each = -(-chunks // want)
    return -(-chunks // each), each, chunks


def family(constants, prefix):
    return (constants[prefix + '_GW_PIX'], constants[prefix + '_GW_WORKGROUPS'],
            constants[prefix + '_GW_MIN_CHUNKS'])


def period_tiles(channels, out_channels):
    """64 output channels x 64 (32 at C = 32) input channels"""
    return (out_channels // 64) * (channels // (32 if channels < 64 else 64))


def generator_tiles(channels):
    """64 (32 at C = 32) output channels x GC_GW_CT input channels"""
    return (channels // (32 if channels < 64 else 64)) * \
        (channels // gconv_oracle.CONSTANTS['GC_GW_CT'])


def frequency_tiles(channels, out_channels):
    """4 / CB blocks of 16 output channels x CB blocks of 16 input channels,
    CB = 1 at C = 16 and 2 above"""
    blocks = 1 if channels == 16 else 2
    return channels // (16 * blocks) * -(-out_channels // (64 // blocks))


def period_bytes(pixels, channels, out_channels, stride):
    # B = 1, period 1: Ho = (H - 1) / s + 1 output rows are the pixels
    return _lib.lib().pm_pconv_workspace_bytes(
        1, channels, out_channels, stride * (pixels - 1) + 1, 1, 5, stride)


def generator_bytes(pixels, channels, kernel):
    return _lib.lib().pm_gconv_workspace_bytes(1, channels, pixels, kernel, 1)


def frequency_bytes(pixels, channels, out_channels, stride):
    # one bin: Fo = 1, the frames are the pixels
    return _lib.lib().pm_fdisc_layer_workspace_bytes(
        1, channels, out_channels, 1, pixels, stride)


# (id, tiles, (PIX, WORKGROUPS, MIN_CHUNKS), floats of a partial,
#  workspace bytes of `pixels` output pixels)
LAYERS = []
for _c, _o, _k, _s in pconv_oracle.FORMS:
    if _c > 1 and _o > 1:
        LAYERS.append((
            f'period-{_c}-{_o}', period_tiles(_c, _o),
            family(pconv_oracle.CONSTANTS, 'PC'), _o * _c * _k + _o,
            lambda pixels, c=_c, o=_o, s=_s: period_bytes(pixels, c, o, s)))
for _c in gconv_oracle.CHANNELS:
    for _k in gconv_oracle.KERNELS:
        LAYERS.append((
            f'generator-{_c}-{_k}', generator_tiles(_c),
            family(gconv_oracle.CONSTANTS, 'GC'), _c * _c * _k + _c,
            lambda pixels, c=_c, k=_k: generator_bytes(pixels, c, k)))
for _c, _o, _s in ((16, 32, 1), (16, 32, 2), (32, 64, 1), (32, 64, 2),
                   (64, 128, 1), (64, 128, 2), (128, 256, 1), (128, 256, 2),
                   (32, 32, 1), (64, 64, 1), (128, 128, 1)):
    LAYERS.append((
        f'frequency-{_c}-{_o}-{_s}', frequency_tiles(_c, _o),
        family(fdisc_strided_oracle.CONSTANTS, 'FS'), _o * (_c + 2) * 9 + _o,
        lambda pixels, c=_c, o=_o, s=_s: frequency_bytes(pixels, c, o, s)))


def test_the_layers_have_the_tile_counts_of_the_three_families():
    tiles = {name: count for name, count, _, _, _ in LAYERS}
    # O 128 ... 1024 at the period layers
    assert [tiles[f'period-{c}-{o}'] for c, o in (
        (32, 128), (128, 512), (512, 1024), (1024, 1024))] == [2, 16, 128, 256]
    # C 32 ... 256 of the generator
    assert [tiles[f'generator-{c}-3'] for c in (32, 64, 128, 256)] == \
        [1, 2, 8, 32]
    # the 16 -> 32 strided layer: one tile, O = 32 under OT = 64
    assert tiles['frequency-16-32-2'] == 1
    assert [tiles[f'frequency-{c}-{2 * c}-2'] for c in (32, 64, 128)] == \
        [2, 8, 32]


@pytest.mark.parametrize('name,tiles,constants,partial,query', LAYERS,
                         ids=[layer[0] for layer in LAYERS])
def test_the_workspace_holds_the_partials_of_the_one_split(
        name, tiles, constants, partial, query):
    pix, workgroups, least = constants
    room = max(workgroups // tiles, 1)
    counts = (1, 2, 3, least * room - 1, least * room, least * room + 1)
    seen = set()
    for chunks in counts:
        # the fewest and the most pixels of that many chunks
        for pixels in ((chunks - 1) * pix + 1, chunks * pix):
            parts, each, got = split(pixels, pix, tiles, workgroups, least)
            assert got == chunks
            assert parts <= room and (parts - 1) * each < chunks <= parts * each
            assert each >= least or parts == 1
            need = -(-parts * partial * 4 // 256) * 256
            assert query(pixels) == need, (name, pixels)
            seen.add(parts)
    # no partial more than the room, and the room is reached
    assert 1 in seen and room in seen
    # (a partial is far more than the 256 bytes of the rounding: the bytes
    # tell the partials apart)
    assert partial * 4 > 256
