"""The cases of test_gpu_out_rows.py, built from exact_oracle.py's parts:
small integers, every sum exact in fp32 and independent of its order.
test_cpu_out_rows_cases.py builds every one and asserts its exactness without
a GPU, so that no case can leave the exact range unnoticed.

(a) PAIR: one Block iteration at C = 256 (conv_pair_kernel). The inputs are
    E.iteration_case's (same seeds); the iteration is computed once per
    (mode, k, d, length) and the three store modes applied to it. Valid
    outputs per tile of the wide geometry: 182 at k 11, 186 at k 7; of the
    latency geometry 54 and 58.
(b) BLOCK: whole Blocks through pm_block_cl / pm_block_act16_cl in the four
    forms that store through pm_store_out_rows or beside it. Lengths: one
    window plus one column, window + 33 (an end inside a wave's second tile)
    and 33 columns - with three forced segments the third segment is empty and
    stores nothing, the second holds one column. (A segment that is not empty
    always stores on its first step: a window is 256 columns or more, halo and
    skew together at most 124.)
(c) MRF: pm_mrf_cl at C = 32 on 769 columns, one 768-column tile plus one.
"""
import functools

import exact_oracle as E

MODES = ('bf16', 'f16')
STORE_MODES = (0, 1, 2)

# (a) ------------------------------------------------------------------------
PAIR_C = 256
PAIR_DILATIONS = (1, 5)
PAIR_LENGTHS = {11: (1, 31, 182, 183, 365), 7: (186, 187, 373)}
PAIR_RAGGED = (365, 183)
# batch 2 takes the latency geometry (two tiles a wave), 75 copies of it the
# wide one (six): the launcher's threshold is 150 workgroups
PAIR_REPLICAS = 75


def pair_table():
    return [(mode, k, d, length) for mode in MODES
            for k, lengths in PAIR_LENGTHS.items() for d in PAIR_DILATIONS
            for length in lengths]


@functools.lru_cache(maxsize=None)
def pair_case(mode, k, d, length):
    c = PAIR_C
    w = E.dense_iteration(c, k, 7 * c + k)
    x = E.dense_input(E.BATCH, c, length, 100 * c + 10 * k + d)
    prev = E.int_fill(E.BATCH, c, length, length + d)
    y, bits = E.block_iteration(x, *w, mode, d)
    want = {m: E.store(y, m, E.SCALES[m], prev) for m in STORE_MODES}
    return dict(x=x, w=w, prev=prev, want=want, bits=bits)


@functools.lru_cache(maxsize=None)
def pair_alone(mode, k, d, length, b, valid):
    """Utterance `b` of pair_case(...), cut to `valid` columns, on its own."""
    case = pair_case(mode, k, d, length)
    y, bits = E.block_iteration(case['x'][b:b + 1, :, :valid], *case['w'],
                                mode, d)
    prev = case['prev'][b:b + 1, :, :valid]
    want = {m: E.store(y, m, E.SCALES[m], prev) for m in STORE_MODES}
    return dict(want=want, bits=bits)


# (b) ------------------------------------------------------------------------
# (c, k, form, window): the forms of E.block_form
BLOCK_SHAPES = ((128, 11, 'skewed', 256), (64, 7, 'skewed', 512),
                (128, 3, 'walked', 256), (64, 3, 'tiled', 256))
REQUEST = {'skewed': 'skewed', 'walked': 'walked', 'tiled': 'own'}


def block_lengths(c):
    window = 256 if c == 128 else 512
    return (window + 1, window + 33, 33)


def block_runs(c, k, form):
    """(mode, niter, dilations, nseg, length, store mode, act16 type | None):
    store modes 1 and 2, act16 as bf16 and as f16 (skewed only) and 1, 2 and
    3 forced segments (the tiled form has none) spread over the lengths."""
    first, second, short = block_lengths(c)
    runs = [('bf16', 1, (5,), 1, first, 2, None),
            ('f16', 2, (1, 3), 2, second, 1, None),
            ('bf16', 2, (3, 5), 3, short, 2, None),
            ('f16', 1, (3,), 3, first, 1, None)]
    if form == 'skewed':
        runs += [('bf16', 1, (1,), 2, first, 2, 'bf16'),
                 ('f16', 2, (5, 1), 3, second, 1, 'f16'),
                 ('bf16', 2, (1, 3), 1, second, 2, 'f16'),
                 ('f16', 1, (5,), 3, short, 1, 'bf16')]
    if form == 'tiled':
        runs = [(m, n, dil, 0, length, sm, act)
                for m, n, dil, _, length, sm, act in runs]
    return runs


def block_table():
    return [(c, k, form, index) for c, k, form, _ in BLOCK_SHAPES
            for index in range(len(block_runs(c, k, form)))]


@functools.lru_cache(maxsize=None)
def block_case(c, k, form, index):
    mode, niter, dilations, nseg, length, store_mode, act = \
        block_runs(c, k, form)[index]
    assert E.block_form(mode, c, k, REQUEST[form]) == form
    seed = 2000 * c + 10 * k + index
    if niter == 1:
        w = tuple([t] for t in E.dense_iteration(c, k, seed))
        x = E.dense_input(E.BATCH, c, length, seed + 1)
    else:
        w = E.sparse_block(c, k, niter, seed, index)
        x = E.sparse_input(E.BATCH, c, length, seed + 1)
    prev = E.int_fill(E.BATCH, c, length, seed + 2)
    y, bits = E.block(x, *w, mode, dilations)
    want = E.store(y, store_mode, E.SCALES[store_mode], prev)
    return dict(mode=mode, x=x, w=w, prev=prev, want=want, bits=bits,
                nseg=nseg, length=length, dilations=dilations,
                store_mode=store_mode, act=act)


# (c) ------------------------------------------------------------------------
MRF_C = 32
MRF_LENGTH = 769
MRF_SEGMENTS = (1, 2)
MRF_RUNS = (('bf16', 1, (3,)), ('f16', 2, (1, 3)))


@functools.lru_cache(maxsize=None)
def mrf_case(index):
    mode, niter, dilations = MRF_RUNS[index]
    blocks = []
    for k in (3, 7, 11):
        seed = 900 * MRF_C + 10 * k + index
        if niter == 1:
            blocks.append(tuple([t] for t in E.dense_iteration(MRF_C, k, seed)))
        else:
            blocks.append(E.sparse_block(MRF_C, k, niter, seed, index))
    x = (E.dense_input if niter == 1 else E.sparse_input)(
        E.BATCH, MRF_C, MRF_LENGTH, 91 * MRF_C + index)
    parts, total, bits = E.mrf_sum(x, blocks, mode, dilations)
    return dict(mode=mode, niter=niter, dilations=dilations, x=x,
                blocks=blocks, parts=parts, total=total, bits=bits)
