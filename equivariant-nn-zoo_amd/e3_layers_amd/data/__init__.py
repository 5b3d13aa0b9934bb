from .data import Data, Batch
from .compute_edge import (PairCriterion, SequenceOrRandom, check_cell, image_ranges, computeEdgeVector, computeEdgeIndex, computeEdgeIndexCapped,
                           wrap_positions)

__all__ = ["Data", "Batch", "PairCriterion", "SequenceOrRandom", "computeEdgeVector", "computeEdgeIndex", "computeEdgeIndexCapped",
           "check_cell", "image_ranges", "wrap_positions"]
