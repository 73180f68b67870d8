#!/usr/bin/env python3
"""What the coordinate-wise trimmed mean costs on one GPU (``profiles/trimmed_mean_bench.md``
quotes the JSON lines this prints).

* ``combine``: the one launch of ``csrc/kernels/trimmed.hip`` at the headline model's flat
  gradient (``bench.py``'s defaults) for ``W`` = 2, 4, 8, 16 sites at ``b = 1`` and at the median,
  by HIP events around replays of a graph that holds one combine, and the effective rate over the
  ``4 (W + 1) n`` bytes it must move.  Beside it the same result formed with torch on the same
  rows in the same process (``torch.sort(dim=0)``, slice, ``sum``, one multiply; finite inputs),
  event-timed eagerly: its sort alone runs for many launch overheads.
* ``step`` (``--step-runs`` > 0): the training step of 3 site processes that share this GPU over
  gloo with ``dsgd_collective=peer`` (the gather captured in the step), ``trimmedMean`` and
  ``dSGD`` in alternating runs.  A rehearsal figure: the sites share one GPU's CUs and HBM.

    python tools/bench_trimmed_mean.py [--reps 200] [--step-runs 2] [--steps 100]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WS = (2, 4, 8, 16)


def _headline_numel(b):
    import torch
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams
    torch.manual_seed(1234)
    model = ICALstm(input_size=b.input_size, hidden_size=b.hidden, num_comps=b.comps,
                    window_size=b.window, num_cls=2)
    return FlatParams(model.parameters()).grad.numel()


def _eager_us(fn, reps):
    import torch
    for _ in range(3):
        fn()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) * 1000.0 / reps


def combine_cost(n, reps):
    import torch
    from bench_topk import _graph_us
    from dinunet_implementations_amd.ops import TrimmedState
    from dinunet_implementations_amd.ops import reference as ref
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows_out = []
    for W in WS:
        for b in sorted({1, ref.trimmed_b(W)} if W > 2 else {ref.trimmed_b(W)}):
            st = TrimmedState("cuda", n, W, b)
            rows = st.gather_buffer()
            rows[:, :n].copy_(torch.randn(W, n, device="cuda", generator=gen) * 1e-2)
            out = torch.empty(n, device="cuda")
            inv = torch.tensor(st.inv, device="cuda")
            base = torch.empty(n, device="cuda")

            def kernel(st=st, rows=rows, out=out):
                st.combine(rows, out)

            def torch_form(rows=rows, base=base, W=W, b=b, inv=inv):
                s = torch.sort(rows[:, :n], dim=0).values[b:W - b].sum(0)
                base.copy_(s if W - 2 * b == 1 else s * inv)

            us = _graph_us(kernel, reps)
            tus = _eager_us(torch_form, max(10, reps // 10))
            nbytes = 4 * (W + 1) * n
            rows_out.append({"W": W, "b": b, "kernel_us": round(us, 2),
                             "kernel_GBps": round(nbytes / us / 1e3, 1),
                             "torch_us": round(tus, 2), "torch_GBps": round(nbytes / tus / 1e3, 1),
                             "speedup": round(tus / us, 2),
                             "max_abs_diff_vs_torch": float((out - base).abs().max())})
    return {"what": "combine", "n": n, "reps": reps, "bytes": "4 (W + 1) n", "rows": rows_out}


def step_worker(engine, steps, warmup):
    """One site process (under torch.distributed.run): host-fed captured steps of the headline
    model, timed after the warm-up by a host clock around work that ends in a synchronise."""
    import torch
    from bench_topk import _bench_defaults
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import init_sites, make_engine, shutdown
    from dinunet_implementations_amd.runtime.step import TrainStep
    b = _bench_defaults()
    grp = init_sites()
    dev = grp.device
    torch.manual_seed(1234)
    model = ICALstm(input_size=b.input_size, hidden_size=b.hidden, num_comps=b.comps,
                    window_size=b.window, num_cls=2).to(dev).train()
    flat = FlatParams(model.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    eng = make_engine(engine, model, flat, grp, {"precision_bits": "32", "seed": 0,
                                                 "dsgd_collective": "peer", "trim_sites": 1})
    step = TrainStep(model, flat, opt, eng, task="ica", use_graph=True)
    S = b.temporal // b.window
    g = torch.Generator(device=dev).manual_seed(100 + grp.rank)
    xs = torch.randn(b.pool, b.batch, S, b.comps, b.window, device=dev, generator=g)
    ys = torch.randint(0, 2, (b.pool, b.batch), device=dev, generator=g)
    for i in range(warmup):
        step(xs[i % b.pool], ys[i % b.pool])
    torch.cuda.synchronize()
    grp.barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        step(xs[i % b.pool], ys[i % b.pool])
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / steps
    all_ms = grp.all_gather_object(ms)
    if grp.rank == 0:
        print(json.dumps({"engine": engine, "world": grp.world, "ms_per_step": max(all_ms),
                          "comm_graph": bool(step.comm_graph), "peer": bool(eng.peer),
                          "n": flat.grad.numel()}), flush=True)
    shutdown()
    return 0


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def step_times(runs, steps, warmup, world=3):
    ms = {"dSGD": [], "trimmedMean": []}
    info = {}
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for _ in range(runs):
        for name in ms:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
                   "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port",
                   str(_free_port()), os.path.abspath(__file__), "--worker", name, "--steps",
                   str(steps), "--warmup", str(warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=170)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                raise RuntimeError(f"step run of {name} failed ({r.returncode}):\n"
                                   f"{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
            res = json.loads(lines[-1])
            ms[name].append(round(res["ms_per_step"], 4))
            info[name] = {k: res[k] for k in ("comm_graph", "peer", "n")}
    return {"what": "step", "world": world, "shared_gpu": True, "collective": "peer",
            "steps": steps, "warmup": warmup, "ms_per_step": ms, "info": info,
            "median": {k: round(statistics.median(v), 4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="timed replays of one combine")
    ap.add_argument("--step-runs", type=int, default=2, help="alternating 3-process runs")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_trimmed_mean.py needs a GPU", file=sys.stderr)
        return 2
    if a.worker:
        return step_worker(a.worker, a.steps, a.warmup)
    from bench_topk import _bench_defaults
    n = _headline_numel(_bench_defaults())
    print(json.dumps(combine_cost(n, a.reps)), flush=True)
    if a.step_runs > 0:
        print(json.dumps(step_times(a.step_runs, a.steps, a.warmup)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
