"""pointnet2_ops.pointnet2_utils surface (reference utils/misc.py:18-19, tools/runner_module.py:151-153,
models/Transformer_utils.py:225-230, and the PointNet++-style models built on the rest of the package), served by the gfx950
kernels of libupp_hip.so."""
from upp_hip.functional import (  # noqa: F401
    FurthestPointSampling, GatherOperation, furthest_point_sample, gather_operation,
    BallQuery, ThreeNN, ThreeInterpolate, GroupingOperation,
    ball_query, three_nn, three_interpolate, grouping_operation, QueryAndGroup, GroupAll,
)

__all__ = ["FurthestPointSampling", "GatherOperation", "furthest_point_sample", "gather_operation",
           "BallQuery", "ThreeNN", "ThreeInterpolate", "GroupingOperation",
           "ball_query", "three_nn", "three_interpolate", "grouping_operation", "QueryAndGroup", "GroupAll"]
