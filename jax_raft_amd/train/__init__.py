"""Training: the fused native step, the sequence loss, data (synthetic, and real datasets with
the fused GPU augmentation) and the data-parallel trainer."""
from .augment import AugmentParams, augment_pairs
from .datasets import FlowPairs, PairLoader

__all__ = ("augment_pairs", "AugmentParams", "FlowPairs", "PairLoader")
