from .data import Data, Batch
from .compute_edge import computeEdgeVector, computeEdgeIndex, computeEdgeIndexCapped

__all__ = ["Data", "Batch", "computeEdgeVector", "computeEdgeIndex", "computeEdgeIndexCapped"]
