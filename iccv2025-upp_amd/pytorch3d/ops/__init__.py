"""pytorch3d.ops: knn_points and knn_gather (README "The pytorch3d.ops surface")."""
from .knn import _KNN, knn_gather, knn_points

__all__ = ["knn_points", "knn_gather"]
