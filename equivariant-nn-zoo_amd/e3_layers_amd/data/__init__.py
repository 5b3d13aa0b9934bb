from .data import Data, Batch
from .compute_edge import PairCriterion, SequenceOrRandom, computeEdgeVector, computeEdgeIndex, computeEdgeIndexCapped

__all__ = ["Data", "Batch", "PairCriterion", "SequenceOrRandom", "computeEdgeVector", "computeEdgeIndex", "computeEdgeIndexCapped"]
