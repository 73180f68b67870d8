#!/usr/bin/env python3
"""What top-k sparsification costs on one GPU, beside the engines it is compared with.

Two measurements in one job (one JSON line each, ``profiles/topk_bench.md`` quotes them):

* ``reduce``: kernel time of one ``engine.reduce()`` at the headline model (``bench.py``'s
  defaults: about 1.06 M parameters) for ``topK`` at ``--ratio`` and for PowerSGD, one site, by
  HIP events around replays of a graph that holds one reduction (no launch overhead in the
  figure); for topK also the select + compact half alone.
* ``step``: the B = 32 training step through ``runtime.feed.DeviceFeed`` exactly as ``bench.py``
  sets it up (its argument defaults are imported, not copied), ``agg_engine`` dSGD and topK in
  alternating runs.

    python tools/bench_topk.py [--ratio 0.01] [--steps 200] [--warmup 30] [--runs 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench_defaults():
    import bench
    argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


def _setup(b, engine, cfg):
    """Model, flat parameters, optimizer and engine as ``bench.main`` builds them."""
    import torch
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    dev = torch.device("cuda")
    torch.manual_seed(1234)
    model = ICALstm(input_size=b.input_size, hidden_size=b.hidden, num_comps=b.comps,
                    window_size=b.window, num_cls=2).to(dev).train()
    flat = FlatParams(model.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    eng = make_engine(engine, model, flat, SiteGroup(device=dev),
                      {"precision_bits": "32", "seed": 0, **cfg})
    return model, flat, opt, eng


def _graph_us(fn, reps):
    """Microseconds of one ``fn()`` on the GPU: a graph of one call, ``reps`` replays between
    two events."""
    import torch
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(5):
        g.replay()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        g.replay()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) * 1000.0 / reps


def reduce_cost(b, ratio, reps):
    import torch
    out = {"what": "reduce", "reps": reps}
    gen = torch.Generator(device="cuda").manual_seed(5)
    for name, cfg in (("topK", {"topk_ratio": ratio}), ("powerSGD", {"powersgd_rank": 4})):
        _, flat, _, eng = _setup(b, name, cfg)
        grad = torch.randn(flat.grad.numel(), device="cuda", generator=gen) * 1e-2

        def one(eng=eng, flat=flat, grad=grad):
            flat.grad.copy_(grad)  # a fresh gradient per release (its copy is timed apart)
            eng.reduce()

        def copy_only(flat=flat, grad=grad):
            flat.grad.copy_(grad)

        total, copy = _graph_us(one, reps), _graph_us(copy_only, reps)
        out[name] = {"reduce_us": round(total - copy, 2), "with_copy_us": round(total, 2),
                     "copy_us": round(copy, 2), "n": flat.grad.numel()}
        if name == "topK":
            def select(eng=eng, flat=flat, grad=grad):
                flat.grad.copy_(grad)
                eng.pre_reduce()
            out[name]["select_us"] = round(_graph_us(select, reps) - copy, 2)
            out[name]["k"] = eng.k
            out[name]["bytes_per_step"] = eng.comm_bytes
    return out


def step_time(b, engine, cfg, steps, warmup):
    import torch
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    from dinunet_implementations_amd.runtime.step import TrainStep
    model, flat, opt, eng = _setup(b, engine, cfg)
    step = TrainStep(model, flat, opt, eng, task="ica", use_graph=True)
    S = b.temporal // b.window
    g = torch.Generator(device="cuda").manual_seed(100)
    xs = torch.randn(b.pool, b.batch, S, b.comps, b.window, device="cuda", generator=g)
    ys = torch.randint(0, 2, (b.pool, b.batch), device="cuda", generator=g)
    K = max(d for d in range(1, 11) if steps % d == 0)
    feed = DeviceFeed(step, xs.view(b.pool * b.batch, S, b.comps, b.window), ys.view(-1), b.batch,
                      nb=b.pool, col=1, steps_per_graph=K)
    del xs
    feed.run(warmup)
    feed.prepare(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    feed.run(steps)
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratio", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=4, help="alternating runs per engine")
    ap.add_argument("--reps", type=int, default=200, help="timed replays of one reduction")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_topk.py needs a GPU", file=sys.stderr)
        return 2
    b = _bench_defaults()
    print(json.dumps(reduce_cost(b, a.ratio, a.reps)), flush=True)
    if a.runs < 1:
        return 0
    ms = {"dSGD": [], "topK": []}
    for _ in range(a.runs):
        for name, cfg in (("dSGD", {}), ("topK", {"topk_ratio": a.ratio})):
            ms[name].append(round(step_time(b, name, cfg, a.steps, a.warmup), 4))
    print(json.dumps({"what": "step", "batch": b.batch, "steps": a.steps, "warmup": a.warmup,
                      "ratio": a.ratio, "ms_per_step": ms,
                      "median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                      "min": {k: min(v) for k, v in ms.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
