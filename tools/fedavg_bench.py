#!/usr/bin/env python3
"""What federated averaging with local steps costs on one GPU (``profiles/fedavg_bench.md`` quotes
the JSON lines this prints).

* ``--mode round``: one whole round (delta launch, the site mean, adopt launch) at the headline
  model's flat parameters (``bench.py``'s defaults), issued eagerly as the site loop issues it,
  timed by device events over ``--reps`` rounds after a warm-up: on a world of one (no
  collective) and, with ``--loopback``, on a one-rank RCCL group (the distributed path: an
  all-reduce and the 1/W multiply between the launches).
* ``--mode kernels --only delta|adopt``: that launch alone ``--reps`` times, for a
  ``rocprofv3 --kernel-trace --stats`` run of its own (the event time it prints includes the
  launch gaps).
* ``--mode step``: the update rate of ``--world`` site processes that share this GPU over gloo,
  device-fed epochs of the headline model: ``fedAvg`` at each ``--local-steps`` value (one-site
  K-step graphs, a round after each segment) against ``dSGD`` with ``dsgd_collective=peer`` (the
  exchange captured in every step), in alternating runs; ms per update per site, medians.  A
  rehearsal figure: the sites share one GPU's CUs and HBM.

    python tools/fedavg_bench.py --mode round [--loopback] [--reps 200]
    python tools/fedavg_bench.py --mode step [--runs 5] [--steps 192]
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


def _setup(grp, engine, cfg):
    import torch
    from bench_topk import _bench_defaults
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    b = _bench_defaults()
    dev = grp.device
    torch.manual_seed(1234)
    model = ICALstm(input_size=b.input_size, hidden_size=b.hidden, num_comps=b.comps,
                    window_size=b.window, num_cls=2).to(dev).train()
    flat = FlatParams(model.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    eng = make_engine(engine, model, flat, grp, {"precision_bits": "32", "seed": 0, **cfg})
    return b, model, flat, opt, eng


def _event_us(fn, reps, warmup=20):
    import torch
    for _ in range(warmup):
        fn()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) * 1000.0 / reps


def round_cost(a):
    import torch
    from dinunet_implementations_amd.parallel import init_sites, shutdown
    grp = init_sites(loopback=a.loopback)
    _, _, flat, _, eng = _setup(grp, "fedAvg", {"fedavg_server_momentum": a.momentum})
    eng.begin()
    flat.data.add_(torch.randn_like(flat.data) * 1e-3)
    st = eng.state
    res = {"what": "round", "n": flat.grad.numel(), "reps": a.reps, "momentum": a.momentum,
           "world_of_one": not grp.distributed, "loopback_rccl": bool(grp.loopback),
           "timing": "device events around eagerly issued rounds, one run"}
    if a.mode == "kernels":
        fn = (lambda: st.delta(1.0)) if a.only == "delta" else (lambda: st.adopt(1.0))
        res.update(what="kernel", kernel=a.only, event_us=round(_event_us(fn, a.reps), 2))
    else:
        res["round_us"] = round(_event_us(eng.round, a.reps), 2)
        res["delta_event_us"] = round(_event_us(lambda: st.delta(1.0), a.reps), 2)
        res["adopt_event_us"] = round(_event_us(lambda: st.adopt(1.0), a.reps), 2)
        res["comm_bytes_per_round"] = eng.comm_bytes // max(1, eng.rounds)
    print(json.dumps(res), flush=True)
    shutdown()
    return 0


def step_worker(a):
    """One site process (under torch.distributed.run): device-fed epochs of ``--steps`` updates,
    one to warm up and capture, then ``--epochs`` timed by a host clock that ends in a
    synchronise."""
    import torch
    from dinunet_implementations_amd.parallel import init_sites, shutdown
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    from dinunet_implementations_amd.runtime.step import TrainStep
    grp = init_sites()
    dev = grp.device
    K = int(a.worker_k)
    if K > 0:
        b, model, flat, opt, eng = _setup(grp, "fedAvg", {"fedavg_local_steps": K,
                                                          "dsgd_collective": a.collective})
        eng.begin()
        step_engine, after = eng.local, eng.round
    else:
        b, model, flat, opt, eng = _setup(grp, "dSGD", {"dsgd_collective": "peer"})
        step_engine, after = eng, None
    step = TrainStep(model, flat, opt, step_engine, task="ica", use_graph=True)
    S = b.temporal // b.window
    g = torch.Generator(device=dev).manual_seed(100 + grp.rank)
    X = torch.randn(b.pool * b.batch, S, b.comps, b.window, device=dev,
                    generator=g).to(torch.bfloat16)
    Y = torch.randint(0, 2, (b.pool * b.batch,), device=dev, generator=g)
    feed = DeviceFeed(step, X, Y, b.batch, a.steps, col=1, segment=K or None)
    order = torch.arange(a.steps * b.batch, device=dev) % X.shape[0]
    feed.run_epoch(order, after=after)  # eager warm-up steps and every capture
    torch.cuda.synchronize()
    grp.barrier()
    t0 = time.perf_counter()
    for _ in range(a.epochs):
        feed.run_epoch(order, after=after)
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / (a.epochs * a.steps)
    all_ms = grp.all_gather_object(ms)
    same = grp.all_gather_object(float(flat.data.double().sum()))
    if grp.rank == 0:
        print(json.dumps({"engine": eng.name, "K": K, "world": grp.world,
                          "ms_per_update": max(all_ms), "peer": bool(eng.peer),
                          "comm_graph": bool(step.comm_graph),
                          "graphs": sorted(k for k in step._dgraphs if isinstance(k, int)),
                          "replicas_equal": len(set(same)) == 1,
                          "rounds": getattr(eng, "rounds", None), "n": flat.grad.numel()}),
              flush=True)
    shutdown()
    return 0


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def step_times(a):
    ks = [0] + [int(k) for k in a.local_steps.split(",")]  # 0: dSGD over the peer exchange
    ms = {k: [] for k in ks}
    info = {}
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for _ in range(a.runs):
        for k in ks:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
                   "--nproc-per-node", str(a.world), "--master-addr", "127.0.0.1",
                   "--master-port", str(_free_port()), os.path.abspath(__file__), "--worker-k",
                   str(k), "--steps", str(a.steps), "--epochs", str(a.epochs), "--collective",
                   a.collective]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=170)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                raise RuntimeError(f"step run K={k} failed ({r.returncode}):\n"
                                   f"{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
            res = json.loads(lines[-1])
            ms[k].append(round(res["ms_per_update"], 4))
            info[k] = {x: res[x] for x in ("engine", "peer", "comm_graph", "graphs",
                                           "replicas_equal", "rounds", "n")}
    name = lambda k: "dSGD(peer)" if k == 0 else f"fedAvg(K={k})"
    return {"what": "step", "world": a.world, "shared_gpu": True, "steps_per_epoch": a.steps,
            "timed_epochs": a.epochs, "runs": a.runs, "fedavg_collective": a.collective,
            "ms_per_update_per_site": {name(k): v for k, v in ms.items()},
            "median": {name(k): round(statistics.median(v), 4) for k, v in ms.items()},
            "info": {name(k): v for k, v in info.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="round", choices=["round", "kernels", "step"])
    ap.add_argument("--only", default="delta", choices=["delta", "adopt"])
    ap.add_argument("--loopback", action="store_true", help="a one-rank RCCL group")
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs per configuration")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--steps", type=int, default=192, help="updates per epoch")
    ap.add_argument("--epochs", type=int, default=2, help="timed epochs per run")
    ap.add_argument("--local-steps", default="1,4,16")
    ap.add_argument("--collective", default="peer",
                    help="dsgd_collective of fedAvg's round (dSGD always runs peer): peer, or "
                         "auto = the gloo all-reduce, staged through the host")
    ap.add_argument("--worker-k", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("fedavg_bench.py needs a GPU", file=sys.stderr)
        return 2
    if a.worker_k is not None:
        return step_worker(a)
    if a.mode == "step":
        print(json.dumps(step_times(a)), flush=True)
        return 0
    return round_cost(a)


if __name__ == "__main__":
    sys.exit(main())
