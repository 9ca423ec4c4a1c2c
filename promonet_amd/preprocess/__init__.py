from .core import *
from . import harmonics
from . import loudness
from . import spectrogram
