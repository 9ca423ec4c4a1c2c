"""Baselines of the reference (promonet/baseline): mel resynthesis with Vocos."""
from . import mels                                             # noqa: F401
