#!/usr/bin/env python3
"""Device time of one secure-aggregation release (``csrc/kernels/secagg.hip``): the mask launches
(quantise + W - 1 ChaCha20 blocks per 8 elements, then the tail block) and the open launch, as a
captured HIP graph replayed back to back and timed with events, at the headline model's flat size
(the ``bench.py`` ICA-LSTM) for W = 2, 4, 8 simulated parties.  The kernels need no peers: rank 0
of W with random keys; the open launch reads the party's own wire (its result means nothing, its
time is the real one).

    python tools/secagg_bench.py [--n ELEMS] [--reps 200] [--worlds 2 4 8]

Prints one JSON line: microseconds per release (mask, open, both) per W.
"""
import argparse
import json
import os
import secrets
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def headline_numel() -> int:
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams
    m = ICALstm(input_size=256, hidden_size=384, num_comps=100, window_size=10, num_cls=2)
    return int(FlatParams(m.parameters()).numel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="fp32 elements (0: the headline model)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4, 8])
    a = ap.parse_args()

    import torch
    from dinunet_implementations_amd.ops import SecAggState
    dev = torch.device("cuda")
    n = a.n or headline_numel()
    g = torch.randn(n, device=dev) * 0.01
    out = torch.empty_like(g)
    res = {"n": n, "reps": a.reps, "us_per_release": {}}

    def timed(fn):
        fn()  # kernels resident before the capture
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        for _ in range(10):
            gr.replay()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            gr.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.reps

    for W in a.worlds:
        s = SecAggState(dev, W, 0, [None] + [secrets.token_bytes(32) for _ in range(W - 1)])
        wire = s.wire_like(g)
        mask = timed(lambda: s.mask_(g, wire))
        opn = timed(lambda: s.open_(wire, out))
        both = timed(lambda: (s.mask_(g, wire), s.open_(wire, out)))
        res["us_per_release"][str(W)] = {"mask": round(mask, 2), "open": round(opn, 2),
                                         "mask+open": round(both, 2)}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
