"""Training: the fused native step, the sequence loss, the label-free loss, its occlusion masks and its
self-supervision,
data (synthetic, and real datasets with the fused GPU augmentation) and the data-parallel trainer."""
from .augment import (AugmentParams, MixedAugmentParams, SparseAugmentParams, augment_pairs, augment_pairs_mixed,
                      augment_pairs_sparse, sample_mixed, sample_sparse)
from .datasets import FlowPairs, MixedFlowPairs, PairLoader, SequentialLoader, SparseFlowPairs
from .occlusion import lands_inside, range_map, visibility_masks
from .selfsup import crop_resize, selfsup_loss, selfsup_loss_reference, selfsup_sums
from .unsup import census_sums, smooth2_sums, unsup_loss, unsup_loss_reference

__all__ = ("augment_pairs", "AugmentParams", "FlowPairs", "PairLoader", "augment_pairs_sparse", "SparseAugmentParams",
           "sample_sparse", "SparseFlowPairs", "MixedFlowPairs", "MixedAugmentParams", "sample_mixed",
           "augment_pairs_mixed", "SequentialLoader", "unsup_loss", "unsup_loss_reference", "census_sums",
           "range_map", "lands_inside", "visibility_masks", "crop_resize", "selfsup_loss", "selfsup_loss_reference",
           "selfsup_sums", "smooth2_sums")
