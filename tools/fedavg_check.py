#!/usr/bin/env python3
"""Federated-averaging rounds across sites on ONE GPU: N ranks (torch.distributed.run,
``DINUNET_BACKEND=gloo``, every rank on cuda:0) train a small ICA-LSTM on rank-specific data
through the production TrainStep -- one-site captured steps on the engine's solo dSGD engine --
and meet in a round after every ``--local-steps``-th update and after the last.

    python -m torch.distributed.run --nproc-per-node 3 --master-addr 127.0.0.1 \\
        tools/fedavg_check.py --collective peer

Before every round each rank all-gathers its parameters, so rank 0 can evaluate the numpy mirror
of the round (``tests/fedavg_ref.py``) from every site's own values:

* every rank's delta and its parameters after the round against the mirror's delta / adopt rule
  fed with the mean the rank actually received, bit for bit (always);
* replicas bit-identical after every round (always);
* ``--collective peer`` on the fp32 wire: the received mean equals the fp32 sum in site order
  times 1/W bit for bit (``mean_bit_exact``);
* any fp32 mean: ``|m - m64| <= 2^-23 sum_s |d_s|`` per element against the fp64 mean of the
  deltas (``--weighting samples``: against the fp64 weighted mean of the parameter differences);
* a 16-bit wire: within the per-element bound ``tests/wire_ref.py`` derives for that wire.

Prints one JSON line (rank 0); exit status 0 iff every check holds.
"""
import argparse
import json
import os
import sys

os.environ.setdefault("DINUNET_BACKEND", "gloo")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPLITS = (3, 5, 8, 4, 7, 6, 9, 2)  # --weighting samples: unequal train-split sizes by rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="32")
    ap.add_argument("--payload", default=None, help="payload_dtype (fp16 | bf16 | fp32)")
    ap.add_argument("--collective", default="auto")
    ap.add_argument("--weighting", default="uniform", choices=["uniform", "samples"])
    ap.add_argument("--local-steps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--server-lr", type=float, default=1.0)
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=4)
    a = ap.parse_args()

    import numpy as np
    import torch
    import fedavg_ref as fr
    import wire_ref as wr
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import init_sites, make_engine, shutdown
    from dinunet_implementations_amd.runtime.step import TrainStep

    grp = init_sites()
    dev = grp.device
    W = grp.world
    torch.manual_seed(1234)  # identical init on every site
    m = ICALstm(input_size=64, hidden_size=128, num_comps=20, window_size=10).to(dev).train()
    m.classifier[0].p = 0.0
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    cfg = {"precision_bits": a.precision, "dsgd_collective": a.collective,
           "fedavg_local_steps": a.local_steps, "fedavg_weighting": a.weighting,
           "fedavg_server_lr": a.server_lr, "fedavg_server_momentum": a.momentum}
    if a.payload:
        cfg["payload_dtype"] = a.payload
    eng = make_engine("fedAvg", m, flat, grp, cfg)
    eng.set_samples(SPLITS[grp.rank % len(SPLITS)])
    eng.begin()
    step = TrainStep(m, flat, opt, eng.local, task="ica", use_graph=True)

    got = {}  # what this rank's round saw: its delta, the mean it received
    delta, adopt = eng.state.delta, eng.state.adopt

    def recording_delta(*args):
        out = delta(*args)
        got["d"] = flat.grad.detach().clone()
        return out

    def recording_adopt(*args):
        got["m"] = flat.grad.detach().clone()
        return adopt(*args)
    eng.state.delta, eng.state.adopt = recording_delta, recording_adopt

    g = torch.Generator(device=dev).manual_seed(100 + grp.rank)  # site-specific data
    rounds = []
    for upd in range(1, a.steps + 1):
        x = torch.randn(a.batch, a.seq, 20, 10, device=dev, generator=g)
        y = torch.randint(0, 2, (a.batch,), device=dev, generator=g)
        step(x, y)
        if not eng.round_due(upd, a.steps):
            continue
        pre = flat.data.detach().cpu()
        anchor = eng.state.anchor.detach().cpu()
        u0 = None if eng.state.u is None else eng.state.u.detach().cpu().numpy().copy()
        eng.round()
        rounds.append({"update": upd, "pre": grp.all_gather(pre), "anchor": anchor, "u0": u0,
                       "d": got["d"].cpu(), "m": got["m"].cpu(),
                       "post": grp.all_gather(flat.data.detach().cpu()),
                       "u": None if eng.state.u is None else eng.state.u.detach().cpu(),
                       "dirty": bool(flat.grad.any()), "drift": eng.drift})
    torch.cuda.synchronize()
    errs = None
    if eng.peer:  # a timed-out wait of the peer exchange (sticky error words)
        from dinunet_implementations_amd.parallel import peer as _peer
        errs = grp.all_gather_object([(ar.me, ar.error()) for ar in _peer.arenas()])

    # ---- every rank judges its own round against the mirror ------------------------------------
    sizes = [SPLITS[r % len(SPLITS)] for r in range(W)]
    ws = fr.site_weights(sizes) if a.weighting == "samples" else [np.float32(1.0)] * W
    wire = eng.wire
    res = {"world": W, "peer": bool(eng.peer), "wire": wire, "collective": a.collective,
           "weighting": a.weighting, "rounds": eng.rounds, "comm_bytes": int(eng.comm_bytes),
           "n": int(flat.grad.numel()), "round_updates": [r["update"] for r in rounds],
           "weights": [float(w) for w in ws], "steps": opt.step_count,
           "captured_update": bool(step.graph_opt), "peer_errors": errs}
    ok = {"replicas": True, "delta_bits": True, "adopt_bits": True, "grad_zero": True,
          "drift": True, "mean_bound": True}
    if eng.peer and wire == "fp32":
        ok["mean_bit_exact"] = True
    worst = 0.0
    for r in rounds:
        an = r["anchor"].numpy()
        ps = [p.numpy() for p in r["pre"]]
        dd = [fr.delta(p, an, w) for p, w in zip(ps, ws)]
        ds = [d for d, _ in dd]
        mine_d, mine_drift = dd[grp.rank]
        mgot = r["m"].numpy()
        ok["replicas"] &= all(torch.equal(p, r["post"][0]) for p in r["post"])
        ok["delta_bits"] &= fr.same_bits(r["d"].numpy(), mine_d)
        a2, p2, u2, _ = fr.adopt(mgot, an, r["u0"], a.server_lr, a.momentum)
        ok["adopt_bits"] &= fr.same_bits(r["post"][grp.rank].numpy(), p2)
        if u2 is not None:
            ok["adopt_bits"] &= fr.same_bits(r["u"].numpy(), u2)
        ok["grad_zero"] &= not r["dirty"]
        ok["drift"] &= abs(r["drift"] - mine_drift) <= 1e-10 * mine_drift
        if "mean_bit_exact" in ok:
            ok["mean_bit_exact"] &= fr.same_bits(mgot, fr.mean_site_order(ds))
        if a.weighting == "samples":  # the fp64 weighted mean of the parameter differences
            tot = float(sum(sizes))
            m64 = sum(float(n) * (p.astype(np.float64) - an.astype(np.float64))
                      for n, p in zip(sizes, ps)) / tot
        else:
            m64 = fr.mean64(ds)
        err = np.abs(mgot.astype(np.float64) - m64)
        if wire == "fp32":
            bound = 2.0 ** -23 * sum(np.abs(d.astype(np.float64)) for d in ds)
        else:
            bound = wr.mean_bound(ds, wire, mgot)
        ok["mean_bound"] &= bool(np.all(err <= bound))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
    if errs is not None and any(code for site in errs for _, code in site):
        ok["replicas"] = False  # a timed-out wait: that round used incomplete data
    res["worst_err_over_bound"] = worst
    flags = torch.tensor([1.0 if v else 0.0 for v in ok.values()], dtype=torch.float64)
    grp.all_reduce(flags, op=torch.distributed.ReduceOp.MIN)  # one rank's failure fails the run
    res["checks"] = {k: bool(v > 0.5) for k, v in zip(ok, flags.tolist())}
    res["ok"] = all(res["checks"].values())
    if grp.rank == 0:
        print(json.dumps(res), flush=True)
    shutdown()
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
