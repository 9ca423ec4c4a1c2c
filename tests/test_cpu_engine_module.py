"""The engine handle's lifetime, written once in model/engine.py: every way
the parameters of HiFiGAN, FARGAN and Vocos can change drops a live engine
exactly once and bumps `_generation`; a module without an engine calls
nothing. No GPU: the library is a recording fake and the handle a number."""
import collections
import ctypes

import pytest
import torch

import promonet_amd
from promonet_amd import _lib, distributed
from promonet_amd.model.engine import EngineModule

VOCODERS = {
    'hifigan': lambda: promonet_amd.model.HiFiGAN(8, 4),
    'fargan': lambda: promonet_amd.model.FARGAN(8, 4),
    'vocos': lambda: promonet_amd.model.Vocos(8, 4)}


class FakeLibrary:
    """Every symbol exists, counts its calls and reports success."""

    def __init__(self):
        self.calls = collections.Counter()

    def __getattr__(self, name):
        def function(*arguments):
            self.calls[name] += 1
            return 0
        return function


@pytest.fixture
def library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(_lib, 'lib', lambda: fake)
    return fake


@pytest.fixture(params=sorted(VOCODERS))
def vocoder(request, library):
    """(abi, module); the fake handle never outlives the fake library"""
    module = VOCODERS[request.param]()
    assert isinstance(module, EngineModule) and module.ABI == request.param
    yield request.param, module
    module._engine = None


def with_engine(module):
    module._engine = ctypes.c_void_p(1)
    module._engine_key = (torch.device('cpu'), module._key())
    return module._generation


def assert_dropped_once(library, abi, module, generation):
    assert library.calls[f'pm_{abi}_destroy'] == 1
    assert set(library.calls) == {f'pm_{abi}_destroy'}
    assert module._engine is None and module._engine_key is None
    assert module._generation == generation + 1


def test_load_state_dict_drops_the_engine(library, vocoder):
    abi, module = vocoder
    generation = with_engine(module)
    module.load_state_dict(module.state_dict())
    assert_dropped_once(library, abi, module, generation)


def test_apply_drops_the_engine(library, vocoder):
    abi, module = vocoder
    generation = with_engine(module)
    module.float()
    assert_dropped_once(library, abi, module, generation)


def test_invalidate_engines_drops_the_engine(library, vocoder):
    abi, module = vocoder
    generation = with_engine(module)
    distributed.invalidate_engines(torch.nn.Sequential(module))
    assert_dropped_once(library, abi, module, generation)


def test_no_engine_nothing_to_drop(library, vocoder):
    abi, module = vocoder
    generation = module._generation
    module.load_state_dict(module.state_dict())
    module.float()
    distributed.invalidate_engines(torch.nn.Sequential(module))
    module._destroy()
    assert not library.calls
    assert module._engine is None and module._generation == generation


def test_engine_needs_gpu_parameters(library, vocoder):
    abi, module = vocoder
    name = type(module).__name__
    with pytest.raises(
            RuntimeError,
            match=f'promonet_amd.model.{name} runs on an AMD GPU only'):
        module.engine()
    assert not library.calls
