"""Dataset preparation (reference: promonet/data). Only augmentation is
here; downloading, formatting and partitioning datasets stay out of scope."""
from . import augment                                          # noqa: F401
