#!/usr/bin/env python3
"""One validation pass at the headline geometry (1,024 subjects, S = 98, H = 384), host loop
against the device-fed pass, and the forward-only recurrence against the storing one.

    python tools/bench_eval.py [--subjects 1024] [--passes 7] [--out FILE.json]

Passes: ``NNTrainer.evaluate`` over a ``DeviceLoader`` at batch 32 (the host path), ``EvalFeed`` at
32, and ``EvalFeed`` at ``eval_batch_size`` 256 and 512 -- all in this one process, each warmed
(graphs captured) and then timed ``--passes`` times; the median wall time (host clock around the
pass, device synchronised) and GPU time (HIP events around the pass) are reported.

Recurrence: ``dn_lstm_fwd`` (storing, with the pre-activation buffer: the training form) against
``dn_lstm_fwd_infer`` at B = 32 and B = 512, median of 50 launches timed with HIP events as
``tools/lstm_time.py`` does.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, passes):
    wall, gpu = [], []
    for _ in range(passes):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(e0.elapsed_time(e1))
    return {"wall_ms": round(statistics.median(wall), 3), "gpu_ms": round(statistics.median(gpu), 3),
            "wall_min_ms": round(min(wall), 3), "wall_max_ms": round(max(wall), 3)}


def bench_passes(subjects, passes):
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.data.loader import DeviceLoader
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    from dinunet_implementations_amd.tasks import get_task
    dev = torch.device("cuda", 0)
    cfg = build_config(overrides={"task_id": "ICA-Classification", "batch_size": 32})
    T, _, _ = get_task(cfg["task_id"])
    tr = T(cache=cfg, state={}, device=dev)
    tr.init_nn(seed=0)
    g = torch.Generator().manual_seed(0)
    X = torch.randn(subjects, 98, 100, 10, generator=g).to(dev)
    Y = torch.randint(0, 2, (subjects,), generator=g).to(dev)
    rows = {}
    host = lambda: tr.evaluate(DeviceLoader(X, Y, 32))["averages"].average  # noqa: E731
    ref = tr.evaluate(DeviceLoader(X, Y, 32))
    host()
    rows["host_b32"] = _timed(host, passes)
    for bs in (32, 256, 512):
        feed = EvalFeed(tr, X, Y, bs)
        feed.prepare()
        got = feed.run()
        if bs == 32:  # the same pass, to the bit
            assert torch.equal(got["out"], ref["out"])
            assert got["averages"].average == ref["averages"].average
        else:
            assert (got["out"] - ref["out"]).abs().max() < 1e-2
        rows[f"feed_b{bs}"] = _timed(feed.run, passes)
        del feed
    return rows


def bench_recurrence(reps=50):
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops.gemm import mm_plain
    from dinunet_implementations_amd.ops.lstm import pack_params, padded_hidden
    dev = "cuda"
    S, I, Hd, ndir = 98, 256, 192, 2
    HD = padded_hidden(Hd)
    GP = 4 * HD
    g = torch.Generator(device=dev).manual_seed(0)
    ps = []
    for _ in range(ndir):
        ps += [torch.randn(4 * Hd, I, device=dev, generator=g) * 0.1,
               torch.randn(4 * Hd, device=dev, generator=g) * 0.1,
               torch.randn(4 * Hd, Hd, device=dev, generator=g) * 0.1,
               torch.randn(4 * Hd, device=dev, generator=g) * 0.1]
    wih_p, bias_p, whh_p, _, _ = pack_params(ps, I, torch.device(dev))
    out = {}
    for B in (32, 512):
        BR = int(_lib.lib().dn_lstm_rows_per_wg(B, Hd))
        Bp = (B + BR - 1) // BR * BR
        x = torch.randn(B * S, I, device=dev, generator=g).to(torch.bfloat16)
        xp = mm_plain(x, wih_p, trans_b=True, out_dtype=torch.bfloat16)
        pre = torch.empty(B * S, ndir * GP, dtype=torch.float32, device=dev)
        c_save = torch.empty(ndir, Bp, S, HD, device=dev)
        hprev = torch.empty(ndir, Bp, S, HD, dtype=torch.bfloat16, device=dev)
        hm = [torch.empty(B, ndir * Hd, device=dev) for _ in range(2)]
        hT, cT = torch.empty_like(hm[0]), torch.empty_like(hm[0])
        st = _lib.stream()

        def store():
            _lib.call("dn_lstm_fwd", xp.data_ptr(), bias_p.data_ptr(), whh_p.data_ptr(), B, S, Hd,
                      ndir, c_save.data_ptr(), hprev.data_ptr(), None, hm[0].data_ptr(), 1.0 / S,
                      hT.data_ptr(), cT.data_ptr(), pre.data_ptr(), 0, 0, st)

        def infer():
            _lib.call("dn_lstm_fwd_infer", xp.data_ptr(), bias_p.data_ptr(), whh_p.data_ptr(), B, S,
                      Hd, ndir, None, hm[1].data_ptr(), 1.0 / S, hT.data_ptr(), cT.data_ptr(), 0, st)

        res = {}
        for name, fn in (("storing_us", store), ("forward_only_us", infer)) * 2:  # A B A B
            ts = []
            for it in range(reps + 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= 5:
                    ts.append(e0.elapsed_time(e1) * 1000)
            res.setdefault(name, []).append(round(statistics.median(ts), 1))
        assert torch.equal(hm[0], hm[1])
        out[f"B{B}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"subjects": a.subjects, "passes": a.passes,
           "pass": bench_passes(a.subjects, a.passes), "recurrence": bench_recurrence()}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
