#!/usr/bin/env python3
"""Secure aggregation check on ONE GPU: N site processes (``torch.distributed.run``, gloo group
for the handle and public-key exchanges only, every rank on cuda:0).

``--mode wire``: the peer exchange's ``u64`` wire (``parallel.peer``, ``peer.hip``) with inputs
near 2^63, so every sum wraps -- eagerly and inside a captured HIP graph replayed with fresh
data, against numpy's uint64 sum; every rank must hold the identical sum and no error word.

``--mode site``: the ICA-LSTM through the production TrainStep with ``secure_agg`` on (``--on 0``:
off), host-fed (``--feed host``) or as device-fed K-step graphs (``--feed device``).  Every release
is recorded (the site's gradient before the mask, the mean after the opening); rank 0 checks each
opened mean bit for bit against ``ops.reference.secagg_mean`` of the sites' gradients, against
their fp64 mean within ``2^-41 + (2^-24 + 2^-52) |m|`` and against the fp32 site-order mean (the
option-off arithmetic, one more fp32 rounding: ``+ 2^-24 |m|``); then every rank's parameters
bit for bit.  The native launchers called are counted by name.

Prints one JSON line (rank 0); exit status 0 iff every check passes.
"""
import argparse
import json
import os
import sys

os.environ.setdefault("DINUNET_BACKEND", "gloo")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wire_mode(a, grp):
    import numpy as np
    import torch
    from dinunet_implementations_amd.parallel import peer
    dev, W, me = grp.device, grp.world, grp.rank
    res = {"mode": "wire", "world": W, "ok": True, "cases": []}

    def site_words(step, rank, n):
        rng = np.random.default_rng(1000 * step + rank)
        # near 2^63: every two-site sum already wraps
        x = rng.integers(2 ** 63 - 2 ** 40, 2 ** 63 + 2 ** 40, n, dtype=np.uint64)
        x[::7] = rng.integers(0, 2 ** 64 - 1, x[::7].size, dtype=np.uint64, endpoint=True)
        return x

    for n in a.sizes:
        pm = peer.mean(grp, dev, n, peer.U64, ("check", n))
        x = torch.empty(n, dtype=torch.int64, device=dev)
        same, exact = True, True

        def check(step):
            nonlocal same, exact
            with np.errstate(over="ignore"):
                want = sum(site_words(step, r, n) for r in range(W))
            got = x.cpu().numpy().view(np.uint64)
            exact = exact and bool(np.array_equal(got, want))
            outs = grp.all_gather(x.cpu())
            same = same and all(torch.equal(t, outs[0]) for t in outs)

        x.copy_(torch.from_numpy(site_words(0, me, n).view(np.int64)))
        pm.run_(x)
        torch.cuda.synchronize()
        check(0)
        xs = torch.empty_like(x)
        gr = torch.cuda.CUDAGraph()
        grp.barrier()
        with torch.cuda.graph(gr):
            x.copy_(xs)
            pm.run_(x)
        for step in range(1, 1 + a.reps):
            xs.copy_(torch.from_numpy(site_words(step, me, n).view(np.int64)))
            gr.replay()
            torch.cuda.synchronize()
            check(step)
        err = pm.ar.error()
        ok = same and exact and err == 0
        res["cases"].append({"n": n, "exact": exact, "replicas_identical": same,
                             "error_word": err, "bytes_sent": pm.bytes_sent, "ok": ok})
        res["ok"] = res["ok"] and ok
    return res


def site_mode(a, grp):
    import torch
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam, _lib, reference
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel import peer as _peer
    from dinunet_implementations_amd.runtime.step import TrainStep

    dev, W = grp.device, grp.world
    calls = {}
    orig_call = _lib.call

    def counting(name, *args):
        key = name
        if name == "dn_peer_launch":
            key = f"dn_peer_launch:type{args[2]}"
        calls[key] = calls.get(key, 0) + 1
        return orig_call(name, *args)
    _lib.call = counting

    torch.manual_seed(1234)  # identical init on every site
    m = ICALstm(input_size=128, hidden_size=384, num_comps=50, window_size=10).to(dev).train()
    m.classifier[0].p = 0.0
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    cfg = {"precision_bits": "32", "seed": 5, "dsgd_collective": a.collective,
           "secure_agg": bool(a.on), "dp_fold": 1}
    eng = make_engine("dSGD", m, flat, grp, cfg)
    res = {"mode": "site", "world": W, "on": bool(a.on), "feed": a.feed,
           "state": eng.sa is not None, "peer": bool(eng.peer), "capturable": bool(eng.capturable)}

    # every release: the site's gradient before the mask, the mean after the opening (device
    # copies; inside a capture they become nodes of the graph, so every pair stays one release's)
    pairs = []
    if eng.sa is not None:
        inner = eng._secagg_reduce

        def recorded():
            own = torch.empty_like(flat.grad)
            own.copy_(flat.grad)
            out = inner()
            mean = torch.empty_like(flat.grad)
            mean.copy_(flat.grad)
            pairs.append((own, mean))
            return out
        eng._secagg_reduce = recorded

    step = TrainStep(m, flat, opt, eng, task="ica", use_graph=True)
    g = torch.Generator(device=dev).manual_seed(100 + grp.rank)  # site-specific data
    xs = [torch.randn(a.batch, a.seq, 50, 10, device=dev, generator=g) for _ in range(a.steps)]
    ys = [torch.randint(0, 2, (a.batch,), device=dev, generator=g) for _ in range(a.steps)]
    if a.feed == "device":
        from dinunet_implementations_amd.ops import DeviceSource
        src = DeviceSource(torch.cat(xs).to(torch.bfloat16), torch.cat(ys), a.batch)
        step.bind(src, steps_per_graph=2)
        step.run(a.steps)
    else:
        for x, y in zip(xs, ys):
            step(x, y)
    torch.cuda.synchronize()
    _lib.call = orig_call

    errs = [ar.error() for ar in _peer.arenas()] if eng.peer else []
    mine = flat.data.detach().cpu()
    allp = grp.all_gather(mine)
    same = all(torch.equal(p, allp[0]) for p in allp)
    res.update(replicas_identical=bool(same), error_words=errs, steps=opt.step_count,
               graph=bool(step.graph is not None or getattr(step, "_dgraphs", None)),
               comm_graph=bool(step.comm_graph),
               secagg_calls=sum(v for k, v in calls.items() if k.startswith("dn_secagg")),
               u64_launches=calls.get("dn_peer_launch:type3", 0),
               f32_launches=calls.get("dn_peer_launch:type2", 0))
    ok = same and not any(errs) and bool(mine.isfinite().all())
    if eng.sa is not None:
        res.update(releases=eng.sa.releases, saturated=eng.sa.saturated,
                   nonfinite=eng.sa.nonfinite, transport=eng.sa_transport, pairs=len(pairs))
        gathered = grp.all_gather_object([(o.cpu(), mn.cpu()) for o, mn in pairs])
        ok = ok and eng.sa.releases == a.steps and eng.sa.nonfinite == 0
        if grp.rank == 0:
            bit, within, near_off, worst = True, True, True, 0.0
            for i in range(len(pairs)):
                owns = [gathered[r][i][0] for r in range(W)]
                want, _, _ = reference.secagg_mean(owns)
                for r in range(W):
                    bit = bit and bool(torch.equal(gathered[r][i][1], want))
                mm = torch.stack(owns).double().mean(0)
                bound = 2.0 ** -41 + (2.0 ** -24 + 2.0 ** -52) * mm.abs()
                d = (want.double() - mm).abs()
                within = within and bool((d <= bound).all())
                worst = max(worst, float((d / bound).max()))
                off = owns[0].clone()
                for o in owns[1:]:
                    off += o
                off *= 1.0 / W
                near_off = near_off and bool(((want.double() - off.double()).abs()
                                              <= bound + 2.0 ** -24 * mm.abs()).all())
            res.update(mean_bit_equal=bit, within_bound=within, worst_over_bound=worst,
                       off_on_within_bound=near_off)
            ok = ok and bit and within and near_off and len(pairs) > 0
    res["ok"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="wire", choices=["wire", "site"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[12, 2060, 300_004],
                    help="wire: words per exchange (multiples of 4)")
    ap.add_argument("--reps", type=int, default=3, help="wire: graph replays with fresh data")
    ap.add_argument("--on", type=int, default=1)
    ap.add_argument("--feed", default="host", choices=["host", "device"])
    ap.add_argument("--collective", default="auto")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=24)
    a = ap.parse_args()

    import torch
    from dinunet_implementations_amd.parallel import init_sites, shutdown
    grp = init_sites()
    res = wire_mode(a, grp) if a.mode == "wire" else site_mode(a, grp)
    flags = torch.tensor([1.0 if res["ok"] else 0.0])
    grp.all_reduce(flags, op=torch.distributed.ReduceOp.MIN)
    res["ok"] = bool(flags.item() > 0.5)
    if grp.rank == 0:
        print(json.dumps(res), flush=True)
    grp.barrier()
    shutdown()
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
