from .data import Data, Batch
from .compute_edge import (PairCriterion, SequenceOrRandom, check_cell, computeEdgeVector, computeEdgeIndex, computeEdgeIndexCapped,
                           wrap_positions)

__all__ = ["Data", "Batch", "PairCriterion", "SequenceOrRandom", "computeEdgeVector", "computeEdgeIndex", "computeEdgeIndexCapped",
           "check_cell", "wrap_positions"]
