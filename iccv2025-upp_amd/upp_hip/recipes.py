"""The full fine-tuning recipes as `loss_fn`s of upp_hip.train.TrainStep (reference cfgs/finetune_modelnet_cls.yaml,
finetune_scan_objonly_cls.yaml, finetune_shapenet55_cls.yaml, finetune_shapenetpart_seg.yaml):

    step = TrainStep(model, tuple(pts.shape), loss_fn=recipes.finetune_cls, inputs=[pts, labels])
    step = TrainStep(model, tuple(pts.shape), loss_fn=recipes.finetune_seg, inputs=[pts, onehot, target])
    loss = step.step_inputs(...)

TrainStep's default `forward_kwargs` switch the prompted models' prompters on; PointTransformer and PointTransformer_seg have none, so
their recipes go through `loss_fn` and call the models plainly.  Neither recipe leaves a torch reduction that may allocate a semaphore (a
memset node once captured) in the step: the losses and the classification accuracy are this library's kernels, and the point accuracy is
summed by upp_nll_mean_fwd's fixed-order passes."""
import torch

from . import ops


def finetune_cls(model, pts, labels):
    """PointTransformer: pts (B,N,3), labels (B,) int64 -> (mean cross-entropy, top-1 accuracy * 100)."""
    return model.get_loss_acc(model(pts), labels)


def point_accuracy(logp, target):
    """logp (R,C) log-probabilities, target (R,) int64 -> the share of rows whose arg-max is the target, * 100 (no gradient)."""
    with torch.no_grad():
        hit = (logp.argmax(-1) == target).to(torch.float32)
        if not hit.is_cuda:
            return hit.mean() * 100.0
        # mean(hit) = -nll_mean(hit as a one-column matrix, column 0): two launches, sums in a fixed order
        return ops.nll_mean_fwd(hit.view(-1, 1), target - target).reshape(()) * -100.0


def finetune_seg(model, pts, onehot, target):
    """PointTransformer_seg: pts (B,N,3), onehot (B,16) object classes, target (B*N,) int64 part labels -> (mean NLL, point accuracy * 100)."""
    logp = model(pts, onehot)
    logp = logp.reshape(-1, logp.shape[-1])
    return model.get_loss(logp, target), point_accuracy(logp, target)
