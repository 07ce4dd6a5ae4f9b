"""Batch-parallel training path on CPU: world_size 2, gloo.  The step driver must give the same
averaged gradients (one flat all-reduce) as a single process on the whole batch, and identical
parameters on every rank after the optimizer step."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _seeded


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup_model(install_oracle=True):
    """install_oracle: put the CPU oracle's grouping into the model's op table for good -- in a spawned rank only.  The test process takes
    the `oracle_ops` fixture instead, which puts the HIP entry points back afterwards: the GPU tests of the same session run on them."""
    import oracle
    from models import build_model_from_cfg, upp_layers
    from upp_hip import functional as HF
    from upp_hip.train import freeze_for_peft
    from utils.config import builtin_cfg
    if install_oracle:
        ops = oracle.torch_ops()
        upp_layers.OPS.update(ops)
        HF.fps_gather = ops["fps_gather"]
    torch.manual_seed(0)
    cfg = builtin_cfg('unify_modelnet_cls').model
    # gather_idx=False reproduces the reference's stride-64-into-stride-74 indexing, which reads rows of
    # OTHER samples of the shard: sharding then changes results by construction.  The DP
    # mechanics are checked with per-sample indices.
    cfg.gather_idx = True
    m = build_model_from_cfg(cfg)
    _seeded.fill(m).eval()          # eval: BatchNorm uses running stats, so sharding the batch is exact
    n = freeze_for_peft(m)
    assert n == 619_176
    return m


def _data():
    pts = _seeded.noisy_clouds(4, 1024, seed=0)
    labels = torch.tensor([1, 7, 30, 12])
    return pts, labels


def _worker(rank, world, port, out_dir):
    sys.path[:0] = [p for p in os.environ["UPP_TEST_PATHS"].split(os.pathsep)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    from upp_hip.train import TrainStep
    from utils import dist_utils
    dist_utils.init_dist('pytorch', backend='gloo')
    assert dist_utils.get_dist_info() == (rank, world)
    model = _setup_model()
    pts, labels = _data()
    sl = slice(rank * 2, rank * 2 + 2)
    ts = TrainStep(model, (2, 1096, 3), use_graph=False)
    assert ts.distributed
    ts.pts.copy_(pts[sl]); ts.labels.copy_(labels[sl])
    ts._forward_backward()
    ts.flat.reduce()                # flat = mean over ranks of [grads..., loss, acc]
    flat_after = ts.flat.flat.clone()
    ts._update()
    loss_mean = dist_utils.reduce_tensor(ts.loss.clone())
    allp = dist_utils.gather_tensor(torch.tensor([float(rank)]))
    assert allp.tolist() == [0.0, 1.0]
    if rank == 0:
        torch.save({"flat": flat_after, "loss_mean": loss_mean,
                    "p": model.cls_head_finetune[8].bias.detach().clone()}, os.path.join(out_dir, "r0.pt"))
    else:
        torch.save({"p": model.cls_head_finetune[8].bias.detach().clone()}, os.path.join(out_dir, "r1.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_gloo_step_matches_single_process(tmp_path, oracle_ops):
    from conftest import ROOT, PKG
    os.environ["UPP_TEST_PATHS"] = os.pathsep.join([os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), PKG])
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "r0.pt")
    r1 = torch.load(tmp_path / "r1.pt")
    assert torch.equal(r0["p"], r1["p"]), "ranks diverged after the optimizer step"

    from upp_hip.train import TrainStep
    model = _setup_model(install_oracle=False)
    pts, labels = _data()
    ts = TrainStep(model, (4, 1096, 3), use_graph=False)
    assert not ts.distributed
    ts.pts.copy_(pts); ts.labels.copy_(labels)
    ts._forward_backward()
    full = ts.flat.flat
    n = ts.flat.numel
    # gradient of the mean CE over 4 clouds == mean of the two half-batch gradients
    np.testing.assert_allclose(r0["flat"][:n].numpy(), full[:n].numpy(), rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(r0["flat"][n].item(), full[n].item(), rtol=1e-5)        # averaged loss slot
    np.testing.assert_allclose(r0["loss_mean"].item(), full[n].item(), rtol=1e-5)


def test_flat_grad_buffer_views_survive_backward():
    from utils.dist_utils import FlatGradAllReduce
    lin = torch.nn.Linear(4, 3)
    frozen = torch.nn.Linear(3, 3)
    for p in frozen.parameters():
        p.requires_grad_(False)
    f = FlatGradAllReduce(list(lin.parameters()) + list(frozen.parameters()))
    assert f.count == 15 and f.numel == 16 and f.flat.numel() == 18         # bias starts on a 16-byte boundary: 12 + 3 -> 16 slots
    assert all(v.data_ptr() % 16 == 0 for v in f.views)
    for _ in range(2):
        f.zero()
        frozen(lin(torch.ones(2, 4))).sum().backward()
        base = f.flat.data_ptr()
        for p in lin.parameters():
            assert base <= p.grad.data_ptr() < base + f.flat.numel() * 4        # still a view of the flat buffer
        assert f.flat[:15].abs().sum() > 0 and float(f.flat[15]) == 0.0
    f.reduce()   # no process group: no-op
    with pytest.raises(ValueError):
        FlatGradAllReduce(frozen.parameters())


_SHARDS = {2: [0, 14, 40], 4: [0, 5, 14, 27, 40]}          # uneven shards: the statistics weigh rows, not ranks


def _sync_bn_worker(rank, world, port, out_dir, cumulative):
    sys.path[:0] = [p for p in os.environ["UPP_TEST_PATHS"].split(os.pathsep)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    from models import upp_layers as L
    from utils import dist_utils
    dist_utils.init_dist('pytorch', backend='gloo')
    L.enable_sync_bn(True)
    assert L.sync_bn_active(True) and not L.sync_bn_active(False)
    torch.manual_seed(3)
    bn = torch.nn.BatchNorm1d(24, momentum=None if cumulative else 0.1)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
    x_all = torch.randn(40, 24) * 2.0 + 0.7
    g_all = torch.randn(40, 24)
    rows = slice(_SHARDS[world][rank], _SHARDS[world][rank + 1])
    x = x_all[rows].clone().requires_grad_(True)
    # no host synchronisation inside the layer: a HIP-graph capture (the multi-GPU step drivers capture their step) refuses .item()
    real_item = torch.Tensor.item
    torch.Tensor.item = lambda self: (_ for _ in ()).throw(RuntimeError("host sync inside synchronised BatchNorm"))
    try:
        L.bump_counter(bn.num_batches_tracked)                      # (as every model call site does in front of _bn_rows)
        y = L._bn_rows(x, bn.train(), True, relu=True)
        (y * g_all[rows]).sum().backward()
        L.bump_counter(bn.num_batches_tracked)
        y2 = L._bn_rows(x.detach() * 0.5 + 1.0, bn, True)          # a second batch: running statistics after two updates
    finally:
        torch.Tensor.item = real_item
    # model level: ONE forward of a layer that runs a BatchNorm moves its counter by ONE, inside the forward's counter scope too (the
    # layer function used to bump on top of its callers: 2 per forward, and a cumulative average over 2k batches -- round-4 advisor)
    conv, bn_m = torch.nn.Conv1d(24, 8, 1), torch.nn.BatchNorm1d(8, momentum=None if cumulative else 0.1)
    L.begin_forward(torch.device('cpu'), True)
    L._pointwise_bn_relu(x_all[rows].detach(), conv, bn_m.train(), True)
    L.end_forward()
    assert int(bn_m.num_batches_tracked) == 1, int(bn_m.num_batches_tracked)
    pooled = L.pooling(x_all[rows].reshape(rows.stop - rows.start, 1, 1, 24).detach(), transform=bn) if not cumulative else y2
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    torch.save({"y": y.detach(), "gx": x.grad, "gw": bn.weight.grad, "gb": bn.bias.grad, "rm": rm, "rv": rv, "pooled": pooled.detach(),
                "count": bn.num_batches_tracked.clone()}, os.path.join(out_dir, "s%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,cumulative", [(2, False), (4, False), (4, True)])
def test_sync_bn_switch_gives_the_single_process_statistics(tmp_path, world, cumulative):
    """`--sync_bn` (reference tools/runner_module.py:50-52): with the switch on, a training-mode BatchNorm over rows normalises with the
    statistics of the rows of ALL ranks -- outputs, input gradients, running statistics and the batch counter equal one process seeing
    every row (also with momentum=None: the cumulative average of nn.BatchNorm); the parameter gradients are rank-local partial sums (the
    step's gradient all-reduce adds them).  World sizes 2 and 4, uneven shards, and no host synchronisation inside the layer."""
    from conftest import ROOT, PKG
    os.environ["UPP_TEST_PATHS"] = os.pathsep.join([os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), PKG])
    mp.spawn(_sync_bn_worker, args=(world, _free_port(), str(tmp_path), cumulative), nprocs=world, join=True)
    r = [torch.load(tmp_path / ("s%d.pt" % k)) for k in range(world)]
    torch.manual_seed(3)
    bn = torch.nn.BatchNorm1d(24, momentum=None if cumulative else 0.1)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
    x_all = (torch.randn(40, 24) * 2.0 + 0.7).requires_grad_(True)
    g_all = torch.randn(40, 24)
    y = torch.relu(bn.train()(x_all))
    (y * g_all).sum().backward()
    y2 = bn(x_all.detach() * 0.5 + 1.0)
    close = lambda a, b: np.testing.assert_allclose(a.numpy(), b.detach().numpy(), rtol=2e-5, atol=2e-6)
    close(torch.cat([r[k]["y"] for k in range(world)]), y)
    close(torch.cat([r[k]["gx"] for k in range(world)]), x_all.grad)
    close(sum(r[k]["gw"] for k in range(world)), bn.weight.grad)
    close(sum(r[k]["gb"] for k in range(world)), bn.bias.grad)
    if cumulative:
        close(torch.cat([r[k]["pooled"] for k in range(world)]), y2)
        close(r[0]["rm"], bn.running_mean); close(r[world - 1]["rv"], bn.running_var)
        assert all(int(r[k]["count"]) == 2 for k in range(world))
        assert all(torch.equal(r[0]["rm"], r[k]["rm"]) and torch.equal(r[0]["rv"], r[k]["rv"]) for k in range(world))
        return
    # (momentum 0.1: the workers went on to the pooling site, which updates the statistics once more -- compare after the same three updates)
    # pooling over groups of one row = 2 x the row (max + mean), normalised with the statistics of all 40 rows
    with torch.no_grad():
        want = torch.nn.functional.batch_norm(2.0 * x_all.detach(), bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, bn.eps)
    close(torch.cat([r[k]["pooled"].reshape(-1, 24) for k in range(world)]), want)
    close(r[0]["rm"], bn.running_mean); close(r[world - 1]["rv"], bn.running_var)
    assert all(torch.equal(r[0]["rm"], r[k]["rm"]) and torch.equal(r[0]["rv"], r[k]["rv"]) for k in range(world))
