"""What model/engine.py owns, on the GPU and for each of HiFiGAN, FARGAN and
Vocos: an engine rebuilt from the same state computes the same bits, two
streams cannot share the one workspace while it is in use, and
`private_workspace()` lends a workspace of its own and gives the shared one
back. Every comparison is `torch.equal`; batch 2 x 12 frames."""
import time

import pytest
import torch

import fargan_step_oracle
import promonet_amd
import restatement as oracle

pytestmark = pytest.mark.gpu

BATCH, FRAMES = 2, 12


class Case:
    """One vocoder: `build()` -> a fresh module holding one fixed state on
    the device, `run(module)` -> its forward over one fixed input."""

    def __init__(self, factory, state, inputs, device):
        self.factory, self.device = factory, device
        self.state = {k: v.clone() for k, v in state.items()}
        self.inputs = [t if t is None else t.to(device) for t in inputs]

    def build(self):
        module = self.factory()
        module.load_state_dict(self.state)
        return module.to(self.device).eval()

    def run(self, module):
        with torch.inference_mode():
            audio = module(*self.inputs)
        assert audio.shape == (BATCH, 1, 256 * FRAMES)
        return audio


@pytest.fixture(scope='module', params=['hifigan', 'fargan', 'vocos'])
def case(request, device, golden_fargan, golden_default):
    gen = torch.Generator().manual_seed(5)
    if request.param == 'hifigan':
        def factory():
            return promonet_amd.model.HiFiGAN(
                promonet_amd.NUM_FEATURES, promonet_amd.GLOBAL_CHANNELS)
        inputs = [
            torch.randn(BATCH, promonet_amd.NUM_FEATURES, FRAMES,
                        generator=gen),
            torch.randn(BATCH, promonet_amd.GLOBAL_CHANNELS, 1, generator=gen)]
        state = factory().state_dict()
    elif request.param == 'fargan':
        def factory():
            return promonet_amd.model.FARGAN(113, 258)
        full = oracle.random_state_fargan(seed=golden_fargan['seed'])
        full['pitch_distribution'] = \
            golden_default['pitch_distribution'].clone()
        state = {k[len('model.'):]: v for k, v in full.items()
                 if k.startswith('model.')}
        # (pitch periods inside the lookback the kernel gathers from)
        inputs = [*fargan_step_oracle.features(BATCH, FRAMES, full, seed=5),
                  None]
    else:
        def factory():
            return promonet_amd.model.Vocos(80, 256)
        inputs = [torch.randn(BATCH, 80, FRAMES, generator=gen) - 4.,
                  torch.randn(BATCH, 256, 1, generator=gen)]
        state = factory().state_dict()
    return Case(factory, state, inputs, device)


def test_rebuilt_engine_is_exact(case):
    module = case.build()
    want = case.run(module)
    assert torch.isfinite(want).all() and want.any()
    assert module._engine is not None
    generation = module._generation
    module.load_state_dict(case.state)
    assert module._engine is None and module._generation == generation + 1
    assert torch.equal(case.run(module), want)
    module.to(case.device)
    assert module._engine is None and module._generation == generation + 2
    assert torch.equal(case.run(module), want)
    assert torch.equal(case.run(case.build()), want)


def spin(device, milliseconds):
    """Keep the current stream busy for about `milliseconds` (a counted spin,
    torch.cuda._sleep). The rate of the counter it reads is measured: it need
    not be the shader clock the device reports."""
    probe = 1_000_000
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda._sleep(probe)                     # (loads the kernel)
    start.record()
    torch.cuda._sleep(probe)
    end.record()
    end.synchronize()
    cycles_per_ms = probe / start.elapsed_time(end)
    torch.cuda._sleep(int(milliseconds * cycles_per_ms))


def test_two_streams_cannot_share_the_workspace(case):
    module = case.build()
    if isinstance(module, promonet_amd.model.FARGAN):
        # (its per-call exchange check would wait for stream A)
        module.check_exchange, module.kernel_mode = False, 1
    case.run(module)                # engine packed, workspace allocated
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(case.device), torch.cuda.Stream(case.device)
    with torch.cuda.stream(a):
        spin(case.device, 50)
        began = time.perf_counter()
        on_a = case.run(module)
    with torch.cuda.stream(b):
        with pytest.raises(RuntimeError, match='owns ONE workspace'):
            case.run(module)
        # the premise: stream A was still inside its spin
        assert not a.query(), time.perf_counter() - began
        torch.cuda.synchronize()
        on_b = case.run(module)
    torch.cuda.synchronize()
    assert torch.equal(on_b, on_a)


def test_private_workspace(case):
    module = case.build()
    want = case.run(module)
    shared = module._workspace
    assert shared is not None
    with module.private_workspace() as holder:
        inside = case.run(module)
        private = module._workspace
        assert private is not None and private is not shared
        assert private.data_ptr() != shared.data_ptr()
    assert module._workspace is shared and holder.tensor is private
    assert torch.equal(inside, want)
    assert torch.equal(case.run(module), want)
