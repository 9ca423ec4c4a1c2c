"""Pitch and loudness data augmentation on the device (reference:
promonet/data/augment): the resampy resamples run as pm_resample_interp, the
loudness shift as pm_loudness_shift."""
from .core import *                                            # noqa: F401,F403
from . import loudness                                         # noqa: F401
from . import pitch                                            # noqa: F401
