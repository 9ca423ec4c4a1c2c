"""Helpers of the FARGAN probe tests (test_cpu_fargan_probe.py,
test_gpu_fargan_probe.py): weight sets at a trained network's scale, the
state as the engine stores it (every stored layer rounded to f16 exactly as
`pm_fargan_pack_kernel` rounds it), a table of teacher-forced single-frame
cases at the pitch-period edges, and planted defects that the tests must be
able to see.

`oracle.random_state_fargan` (orthogonal Linear weights, U(-1/16, 1/16) GRU
weights) started from zero state keeps every pre-activation below 1 and every
GRU state below 0.2: the kernels' sigmoid / tanh run around zero only and a
wrong hidden unit is attenuated to nothing before the audio. Scaling the
weights and running many frames is no way out - the scaled network is chaotic
(GRU and gate weights x 8: the oracle's own fp32 and fp64 runs differ by 0.9
after 12 frames, x 4 by 9.5e-4 after 40). ONE frame (4 dependent sub-frame steps) from given O(1)
states is stable, and exposes the states directly."""
import contextlib
from unittest import mock

import torch

import fargan_step_oracle
import restatement as oracle

P = 'model.subframe_network.'
CONDITIONING = tuple(f'model.conditioning_network.{i}' for i in (0, 2, 4))
FWCONV = P + 'framewise_convolution.model.0'
FWCONV_GLU = P + 'framewise_convolution.model.2.gate'
GRU = tuple(P + f'gru{n}.weight_{side}' for side in ('ih', 'hh')
            for n in (1, 2, 3))
GRU_GLU = tuple(P + f'gru{n}_glu.gate' for n in (1, 2, 3))
SKIP = P + 'skip_dense'
SKIP_GLU = P + 'skip_glu.gate'
OUT = P + 'output_layer'

# prefix -> weight-normed; the order of fargan_layers() (pm_fargan.hip)
NORMED = (FWCONV, FWCONV_GLU) + GRU_GLU + (SKIP_GLU,)
GATES_GLU = (FWCONV_GLU,) + GRU_GLU + (SKIP_GLU,)
DENSE = CONDITIONING + (FWCONV, SKIP, OUT)
# stored f16 under 'mixed' (`insensitive` in fargan_layers()): the framewise
# GLU gate, the six GRU matrices, the GRU GLU gates, the skip GLU gate
INSENSITIVE = (FWCONV_GLU,) + GRU + GRU_GLU + (SKIP_GLU,)
SENSITIVE = CONDITIONING + (FWCONV, SKIP, OUT)
STATE_SIZES = (256, 256, 256, 260)

# the pitch-period edges: both ends of the lookback index (512 - p - 2 >= 0
# at 510; the wrapped index 512 - p + 65 - p < 512 at 33), the wrap boundary
# (indices reach 512 for p <= 65 only), ties of rintf / torch.round (64.5 ->
# 64 wraps, 65.5 -> 66 does not, 127.5 -> 128), powers of two, FMIN's 441
PERIOD_EDGES = (33., 65., 510., 40., 64.5, 65.5, 66., 67., 127.5, 128.,
                255., 256., 441., 509.)
BATCHES = (3, 37, 70)


# Gates of test_gpu_fargan_probe.py: <= 3x what MI355X measures (in brackets:
# fp32, mixed, f16; the worst of both kernels and of the batches of 3, 37 and
# 70; profiles/fargan_probe/NOTES.md has every figure). The reference is the
# oracle on the stored weights, so all three storage types do the same fp32
# arithmetic and get the same gate, the smallest of the three 3x figures.
# test_cpu_fargan_probe.py::test_sensitivity holds every f16 / mixed gate
# within 4x the fp32 gate of its kind and the teacher-forced gates below the
# smallest effect of a planted defect (audio 6.9e-5, states 1.0e-3).
GATES = {
    # one teacher-forced frame, 'trained' and 'overflow' weights
    # (audio 1.29e-6, 1.24e-6, 1.04e-6; states 8.1e-6, 7.7e-6, 8.2e-6)
    'trained': {
        'audio': {'fp32': 3e-6, 'mixed': 3e-6, 'f16': 3e-6},
        'states': {'fp32': 2.3e-5, 'mixed': 2.3e-5, 'f16': 2.3e-5}},
    # ... random-init weights (audio 2.05e-7, 2.15e-7, 2.13e-7; states
    # 7.2e-7, 7.2e-7, 3.8e-7)
    'init': {
        'audio': {'fp32': 6e-7, 'mixed': 6e-7, 'f16': 6e-7},
        'states': {'fp32': 2e-6, 'mixed': 2e-6, 'f16': 1.1e-6}}}
GATES['overflow'] = GATES['trained']
# full forward at random init, up to 60 frames (2.17e-7, 2.34e-7, 2.10e-7)
FORWARD_GATES = {'fp32': 6e-7, 'mixed': 6e-7, 'f16': 6e-7}
# 10 frames from zero state: previous samples (1.83e-7, 1.73e-7, 1.57e-7) and
# states (6.2e-7, 6.2e-7, 3.1e-7)
STREAM_GATES = {
    'audio': {'fp32': 4.5e-7, 'mixed': 4.5e-7, 'f16': 4.5e-7},
    'states': {'fp32': 1.8e-6, 'mixed': 1.8e-6, 'f16': 9e-7}}


def key(prefix):
    """The state-dict key of a layer's plain weight."""
    return prefix if prefix.endswith(('_ih', '_hh')) else prefix + '.weight'


LAYERS = CONDITIONING + (FWCONV, FWCONV_GLU) + GRU + GRU_GLU + (
    SKIP, SKIP_GLU, OUT)


def _scale(state, prefix, factor):
    if prefix in NORMED and prefix + '.weight_g' in state:
        state[prefix + '.weight_g'] = state[prefix + '.weight_g'] * factor
    else:
        state[key(prefix)] = state[key(prefix)] * factor


def scaled_state(state, gru=1., glu=1., dense=1.):
    """The reference-keyed state with the GRU matrices, every GLU gate and
    the dense layers (conditioning network, framewise conv, skip dense,
    output layer) multiplied; weight-normed layers through weight_g."""
    state = dict(state)
    for group, factor in ((GRU, gru), (GATES_GLU, glu), (DENSE, dense)):
        for prefix in group:
            _scale(state, prefix, factor)
    return state


def scaled_rows(state, prefix, rows, factor):
    """`rows` of one layer multiplied (weight_g of a normed layer)."""
    state = dict(state)
    name = prefix + '.weight_g' if prefix in NORMED else key(prefix)
    tensor = state[name].clone()
    tensor[rows] *= factor
    state[name] = tensor
    return state


def folded_state(state, fold=oracle.fold_weight_norm_linear):
    """Every weight-normed layer as a plain `.weight` (fp32, `fold`'s bits)."""
    state = dict(state)
    for prefix in NORMED:
        if prefix + '.weight_g' in state:
            g = state.pop(prefix + '.weight_g')
            v = state.pop(prefix + '.weight_v')
            state[prefix + '.weight'] = fold(g, v)
    return state


def stored(dtype):
    """The layers stored as f16 under a weight_dtype."""
    return {'fp32': (), 'mixed': INSENSITIVE, 'f16': LAYERS}[dtype]


def rounded_state(state, dtype, fold=oracle.fold_weight_norm_linear,
                  layers=None):
    """The state whose weights are the values the engine computes with:
    weight norm folded in fp32, then every layer stored as f16 under `dtype`
    rounded to nearest-even as `(_Float16)` does. `layers` overrides the set
    of rounded layers (the planted defects)."""
    state = folded_state(state, fold)
    for prefix in stored(dtype) if layers is None else layers:
        state[key(prefix)] = state[key(prefix)].half().float()
    return state


###############################################################################
# Weight sets
###############################################################################

# Set (b): the largest of the GRU / GLU scales 2, 3, 4, 6 at which one frame
# from O(1) states is both saturated (5 % of the GRU gate pre-activations
# beyond +-4: 0.9 % at x 4, 11.6 % at x 6) and still stable (the oracle's own
# fp32-versus-fp64 difference within NOISE_CAP: audio 2.0e-6, states 1.4e-5 at
# x 6; 6.9e-6 and 7.1e-5 at x 8). test_cpu_fargan_probe.py holds both.
TRAINED_SCALE = 6
NOISE_CAP = {'audio': 5e-6, 'states': 2e-5}
SEED = 5


def base_state(seed=SEED):
    return oracle.random_state_fargan(seed=seed)


def trained_state(state, scale=TRAINED_SCALE, seed=SEED):
    """GRU matrices and GLU gates x `scale`, dense layers as initialised; the
    weight_g of every normed layer takes a per-row factor in U(.75, 1.25) on
    top (at initialisation g = |v| and the fold is the identity: a wrong fold
    would not show)."""
    state = scaled_state(state, gru=scale, glu=scale, dense=1.)
    gen = torch.Generator().manual_seed(seed + 300)
    for prefix in NORMED:
        g = state[prefix + '.weight_g']
        state[prefix + '.weight_g'] = g * (
            .75 + .5 * torch.rand(g.shape, generator=gen))
    return state


# Units pushed past the ends of the kernel's activations: e^(2 v) overflows
# fp32 beyond |v| = 44.4 in fg_tanh, e^(-v) beyond 88.7 in fg_sigmoid. Row r of
# the conditioning network's first layer and of every GLU gate is replaced by
# K e_r: the pre-activation is K x_r, one product with nothing to cancel, so
# no summation order can move it. A saturated unit has zero slope; the gated
# unit x_r sigmoid(K x_r) has a slope below 1.1 for any K (where the sigmoid is
# steep, around x_r = 0, the unit itself is ~0): the set adds no chaos to (b).
# (Whole rows x 256 instead are dot products of 371 terms, 2 800 in absolute
# sum, that cancel to ~0 in the units on tanh's slope: any fp32 summation
# order is off by ~4e-4 there, 2e-5 after the tanh. MI355X measured the fp32
# cluster kernel, whose conditioning GEMM adds the terms in one chain, at
# 5.0e-6 in the audio and 2.6e-5 in the states with such rows, 0.9e-6 and
# 8e-6 elsewhere: a test of the set's conditioning, not of fg_tanh.)
OVERFLOW_ROWS = tuple(range(0, 371, 23))            # 17 rows; 12 below 256
OVERFLOW_TANH = 100.
OVERFLOW_SIGMOID = 200.


def overflow_state(state, scale=TRAINED_SCALE, seed=SEED):
    state = trained_state(state, scale, seed)
    rows = list(OVERFLOW_ROWS)
    weight = state[key(CONDITIONING[0])].clone()
    weight[rows] = OVERFLOW_TANH * torch.eye(weight.shape[1])[rows]
    state[key(CONDITIONING[0])] = weight
    rows = [r for r in OVERFLOW_ROWS if r < 256]
    for prefix in GATES_GLU:
        g = state[prefix + '.weight_g'].clone()
        v = state[prefix + '.weight_v'].clone()
        g[rows] = OVERFLOW_SIGMOID
        v[rows] = torch.eye(256)[rows]
        state[prefix + '.weight_g'], state[prefix + '.weight_v'] = g, v
    return state


WEIGHT_SETS = {
    'init': lambda state: dict(state),
    'trained': trained_state,
    'overflow': overflow_state,
}


###############################################################################
# Teacher-forced cases
###############################################################################

def cases(seed=SEED, state=None):
    """batch size -> (features (B, 114), globals (B, 258), previous samples
    (B, 1, 512) in U(-.95, .95), states in U(-1, 1)): the first B rows of one
    70-row table, whose first 14 rows carry PERIOD_EDGES (the first three are
    both ends and the wrap boundary, so the batch of 3 has them) and whose
    other rows keep synthetic_inputs' periods."""
    state = base_state(seed) if state is None else state
    rows = max(BATCHES)
    features, g = fargan_step_oracle.features(rows, 1, state, seed=seed + 100)
    features = features[:, :, 0].clone()
    features[:len(PERIOD_EDGES), -1] = torch.tensor(PERIOD_EDGES)
    gen = torch.Generator().manual_seed(seed + 200)
    previous = (torch.rand(rows, 1, 512, generator=gen) * 2 - 1) * .95
    states = tuple(torch.rand(rows, n, generator=gen) * 2 - 1
                   for n in STATE_SIZES)
    return {batch: (features[:batch], g[:batch], previous[:batch],
                    tuple(s[:batch] for s in states)) for batch in BATCHES}


def run_oracle(state, case, dtype=torch.float64):
    """One teacher-forced frame of the CPU oracle in `dtype` arithmetic on a
    state with plain or weight-normed layers -> (audio (B, 256), previous
    (B, 1, 512), states 4-tuple)."""
    weights = {k: v.to(dtype) for k, v in oracle.fargan_weights(state).items()}
    features, g, previous, states = case
    with torch.inference_mode():
        return fargan_step_oracle.fargan_step(
            weights, features.to(dtype), g.to(dtype), previous.to(dtype),
            tuple(s.to(dtype) for s in states))


def run_oracle_stream(state, features, g, dtype=torch.float64):
    """`features` (B, 114, T) from zero state and zero previous samples ->
    (audio (B, 1, 256 T), previous (B, 1, 512), states)."""
    weights = {k: v.to(dtype) for k, v in oracle.fargan_weights(state).items()}
    batch = features.shape[0]
    with torch.inference_mode():
        return fargan_step_oracle.fargan_stream(
            weights, features.to(dtype), g.to(dtype),
            torch.zeros(batch, 1, 512, dtype=dtype),
            tuple(torch.zeros(batch, n, dtype=dtype) for n in STATE_SIZES))


def difference(a, b):
    """(audio, states) max-abs difference of two run_oracle results; the
    returned previous samples count as audio."""
    audio = max((a[0].double() - b[0].double()).abs().max().item(),
                (a[1].double() - b[1].double()).abs().max().item())
    states = max((x.double() - y.double()).abs().max().item()
                 for x, y in zip(a[2], b[2]))
    return audio, states


@contextlib.contextmanager
def preactivations():
    """Records what the oracle feeds its activations during one
    `fargan_step`: taps['tanh'] / taps['sigmoid'] lists in call order. Per
    frame 3 conditioning tanh; per sub-frame tanh = framewise conv, n of GRU
    1..3, skip, output and sigmoid = framewise GLU, (r, z, GLU) of GRU 1..3,
    skip GLU."""
    taps = {'tanh': [], 'sigmoid': []}
    real = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid}

    def tap(name):
        def function(x):
            taps[name].append(x.detach().clone())
            return real[name](x)
        return function
    with mock.patch.object(torch, 'tanh', tap('tanh')), \
            mock.patch.object(torch, 'sigmoid', tap('sigmoid')):
        yield taps


def gru_gate_preactivations(taps):
    """The r and z pre-activations of the three GRU cells over the frame."""
    picked = []
    for sub in range(oracle.FARGAN_SUBFRAMES):
        calls = taps['sigmoid'][11 * sub:11 * (sub + 1)]
        for n in range(3):
            picked += calls[1 + 3 * n:3 + 3 * n]
    return torch.cat([t.flatten() for t in picked])


###############################################################################
# Planted defects: state -> the state a subtly wrong engine would compute with
###############################################################################

def _truncate(w):
    """fp32 -> f16 towards zero instead of to nearest."""
    t = w.half()
    bits = t.view(torch.int16)
    over = t.float().abs() > w.abs()
    return torch.where(over, bits - 1, bits).view(torch.float16).float()


def truncated(state, dtype, fold):
    """gru1.weight_ih truncated, not rounded."""
    name = key(GRU[0])
    out = rounded_state(state, dtype, fold)
    out[name] = _truncate(folded_state(state, fold)[name])
    return out


def v_rounded_before_fold(state, dtype, fold):
    """weight_v of the GRU GLU gates rounded, then folded (the stored weight
    is g v16 / |v16|, no f16 value)."""
    state = dict(state)
    for prefix in GRU_GLU:
        state[prefix + '.weight_v'] = state[prefix + '.weight_v'].half().float()
    layers = [l for l in stored(dtype) if l not in GRU_GLU]
    return rounded_state(state, dtype, fold, layers)


def insensitive_left_fp32(state, dtype, fold):
    """'mixed': the framewise GLU gate kept fp32."""
    return rounded_state(state, dtype, fold,
                         [l for l in stored(dtype) if l != FWCONV_GLU])


def sensitive_rounded(state, dtype, fold):
    """'mixed': the skip dense layer stored f16."""
    return rounded_state(state, dtype, fold, list(stored(dtype)) + [SKIP])


def k_slice_unrounded(state, dtype, fold):
    """Columns 64:96 of gru2_glu.gate - cluster member 2's K-split slice -
    left unrounded."""
    name = key(GRU_GLU[1])
    out = rounded_state(state, dtype, fold)
    out[name] = out[name].clone()
    out[name][:, 64:96] = folded_state(state, fold)[name][:, 64:96]
    return out


def gru3_unit_255(state, dtype, fold):
    """The r, z, n rows of unit 255 of gru3.weight_hh (the last row of the
    last cluster member's slice) x 1.001."""
    name = key(GRU[5])
    state = dict(state)
    state[name] = state[name].clone()
    state[name][[255, 511, 767]] *= 1.001
    return rounded_state(state, dtype, fold)


def gru2_member_edges(state, dtype, fold):
    """Rows 0 and 31 of gru2.weight_ih (the edges of a member's 32 units)
    x 1.001."""
    name = key(GRU[1])
    state = dict(state)
    state[name] = state[name].clone()
    state[name][[0, 31]] *= 1.001
    return rounded_state(state, dtype, fold)


# name -> (function, storage types under which it is a defect, the output
# it is meant to show in)
DEFECTS = {
    'truncated': (truncated, ('f16', 'mixed'), 'states'),
    'v_rounded_before_fold': (v_rounded_before_fold, ('f16', 'mixed'),
                              'audio'),
    'insensitive_left_fp32': (insensitive_left_fp32, ('mixed',), 'audio'),
    'sensitive_rounded': (sensitive_rounded, ('mixed',), 'audio'),
    'k_slice_unrounded': (k_slice_unrounded, ('f16', 'mixed'), 'audio'),
    'gru3_unit_255': (gru3_unit_255, ('fp32', 'mixed', 'f16'), 'states'),
    'gru2_member_edges': (gru2_member_edges, ('fp32', 'mixed', 'f16'),
                          'states'),
}
