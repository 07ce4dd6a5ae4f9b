"""Evaluation throughput: eager `validate` / `test_vote` (utils/evaluate.py) against their captured, vote-batched forms
(`validate_captured` / `test_vote_captured`, upp_hip/infer.py) on a seeded unify_modelnet_cls model at ModelNet shapes (B = 32 clouds of
N_raw = 8192 points, npoints 1024, superset 1200, V = 10 votes).  Prints ONE JSON line: per path the first call (warm-up; includes the
capture), the median / min / max ms per batch over the repeats, clouds/s, and the host-side launches per batch (torch profiler: runtime
launch calls, a graph launch counting one) with the kernels they ran.  `test_vote_captured` runs one vote per forward inside the graph
(this recipe's forward reads across samples: upp_hip.infer.mixes_samples); `forward_of_votes_x_B` says what a single forward of all V*B
clouds would meet (the propagation step's 15,360-row limits).
   python tools/eval_throughput.py [--batches 3] [--repeats 5] [--votes 10]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
import torch  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _launches(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    calls = kernels = 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CPU and "launch" in e.name.lower() and e.name.lower().startswith(("hip", "cuda")):
            calls += 1
        elif e.device_type == torch.autograd.DeviceType.CUDA:
            kernels += 1
    return calls, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-raw", type=int, default=8192)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--votes", type=int, default=10)
    a = ap.parse_args()
    import bench
    from utils import evaluate
    from utils.synthetic import noisy_clouds
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev).eval()
    B, nb, V = a.batch, a.batches, a.votes
    batches = [(noisy_clouds(B, a.n_raw, seed=i).to(dev), torch.randint(0, 40, (B,), generator=torch.Generator().manual_seed(i)).to(dev))
               for i in range(nb)]
    gen = torch.Generator(device=dev)

    def run(name):
        gen.manual_seed(0)
        if name == "validate":
            return evaluate.validate(model, batches, 1024)
        if name == "validate_captured":
            return evaluate.validate_captured(model, batches, 1024)
        if name == "test_vote":
            return evaluate.test_vote(model, batches, 1024, times=V, generator=gen)
        return evaluate.test_vote_captured(model, batches, 1024, times=V, generator=gen)

    out = {"B": B, "n_raw": a.n_raw, "npoints": 1024, "superset": 1200, "votes": V, "batches_per_call": nb, "repeats": a.repeats}
    from upp_hip.infer import mixes_samples
    out["one_vote_per_forward"] = mixes_samples(model)
    for name in ("validate", "validate_captured", "test_vote", "test_vote_captured"):
        first = _timed(lambda: run(name)) / nb
        ms = [_timed(lambda: run(name)) / nb for _ in range(a.repeats)]
        calls, kernels = _launches(lambda: run(name))
        med = statistics.median(ms)
        out[name] = {"warmup_ms_per_batch": round(first, 3), "ms_per_batch": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
                     "clouds_per_s": round(B / med * 1e3, 1), "launch_calls_per_batch": round(calls / nb, 1),
                     "kernels_per_batch": round(kernels / nb, 1), "accuracy": float(run(name))}
    out["speedup_validate"] = round(out["validate"]["ms_per_batch"] / out["validate_captured"]["ms_per_batch"], 2)
    out["speedup_test_vote"] = round(out["test_vote"]["ms_per_batch"] / out["test_vote_captured"]["ms_per_batch"], 2)
    P = model.blocks.blocks[0].downstream_prompts.shape[0]
    G = int(model.config.num_group)
    Lp = 1 + G + P
    # which propagation form a forward of V*B clouds would take: the fused HF.propagate stops at B*Lp <= 15360 token rows, and the
    # propagation index (upp_csr_build, rows <= 15360) refuses such a forward altogether -- a reason besides mixes_samples for the chunks
    out["forward_of_votes_x_B"] = {"clouds": V * B, "token_rows": V * B * Lp, "fused_propagate": V * B * Lp <= 15360,
                                   "servable": V * B * Lp <= 15360, "rows_per_forward_run": B * Lp}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
