from . import discriminator
from .core import get_padding
from .fargan import FARGAN, initialize_recurrent_state
from .generator import Generator, MelGenerator
from .hifigan import HiFiGAN, HiFiGANStream, hifigan_context, stream_schedule
from . import hifigan_train
from .hifigan_train import Block, HiFiGANTrainable, ResidualBlock, block_conv
from .vocos import Vocos
