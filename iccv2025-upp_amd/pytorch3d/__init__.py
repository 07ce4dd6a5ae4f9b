"""Drop-in for the part of pytorch3d the reference imports (`import pytorch3d.ops`, models/Point_MAE_pretask_dev.py:20,680):
pytorch3d.ops.knn_points and knn_gather on the kernels of libupp_hip.so (include/upp_hip.h "the pytorch3d.ops surface").

Upstream's kernels are CUDA-only; this package imports on a host without a GPU, like knn_cuda.  The rest of pytorch3d is not here."""
__version__ = "0.7+upp_hip"
