"""Bit-level record of the fused Adam: the cases, the runner and ``--record PATH``.

Every case runs a few updates of one step form with one combination of clipping, schedule and
weight average, and hashes everything the launches wrote.  Only ``FlatParams`` / ``FusedAdam``'s
public API is used, so this file runs unchanged on an older checkout; inputs come from seeded CPU
generators, so they do not depend on the device RNG.  ``tests/golden/adam_bits.json`` is recorded
with it from the commit BEFORE a change to ``optim.hip`` and ``tests/test_adam_bits_gpu.py`` holds
the changed code to it::

    python tests/adam_bits.py --record tests/golden/adam_bits.json --commit <parent id>
"""
import argparse
import hashlib
import itertools
import json
import math
import os
import subprocess
import sys

import torch
import torch.nn as nn

DEV = "cuda"
N = 2053  # 513 float4 (more than one 256-thread workgroup) and a one-element scalar tail
FORMS = ("step", "graphable", "prebumped", "pack")
SCALES = (1.0, 0.02, 3.0)  # of the three gradients: around the threshold, below it, above it
# cosine, warmup 2, lr_min at update 5: three updates cross the warmup and enter the decay
SCHEDULE = dict(kind="cosine", warmup_steps=2, decay_steps=5, lr_min=1e-3)
SWITCHES = ("DINUNET_EMA_DECAY", "DINUNET_LR_SCHEDULE", "DINUNET_MAX_GRAD_NORM")


def cases():
    """``{name: (form, clip, sched, ema, kind)}``; kind: ``updates`` (three of them), ``skip`` (the
    second gradient non-finite, clipping on) or ``prime`` (one update, then a priming launch)."""
    out = {}
    for form, (clip, sched, ema) in itertools.product(FORMS, itertools.product((0, 1), repeat=3)):
        out[f"{form}-clip{clip}-sched{sched}-ema{ema}"] = (form, clip, sched, ema, "updates")
    for form in FORMS:
        out[f"{form}-skip"] = (form, 1, 1, 1, "skip")
    out["pack-prime"] = ("pack", 0, 1, 1, "prime")
    return out


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _build(form, clip, sched, ema):
    """``(flat, opt, tensors to hash, gradient scale, threshold)``.  The pack form updates the
    small ICA model with its persistent pack attached; the others a vector of N elements sliced
    from a padded buffer, whose padding is hashed too."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    if form == "pack":
        from dinunet_implementations_amd.models import ICALstm
        torch.manual_seed(0)  # (the CPU generator: the model is built there)
        m = ICALstm(input_size=64, hidden_size=128, num_comps=20, window_size=10).cuda().train()
        flat, base, c = FlatParams(m.parameters()), 1e-2, 1.0
    else:
        flat, base, c = FlatParams([nn.Parameter(_randn(N + 3, 1).to(DEV))]), 1.0, 10.0
    opt = FusedAdam(flat, lr=1e-2, weight_decay=1e-4, max_grad_norm=c if clip else 0,
                    lr_schedule=dict(SCHEDULE) if sched else None, ema_decay=0.9 if ema else 0)
    keep = {"data": flat.data, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq,
            "grad": flat.grad}
    if ema:
        keep["ema"] = opt.ema
    if form == "pack":
        pp = m.persistent_pack(flat.data.device)
        opt.attach_pack(pp)
        for i, t in enumerate([pp.wih_p, pp.bias_p, pp.whh_p, pp.whhT_p] + pp.casts + pp.extra):
            keep[f"image{i}"] = t
    else:
        # (the gradient keeps its padded length: the norm kernel of a clipped update takes
        # whole float4s only, and the update reads the first N of it)
        flat.data = flat.data[:N]
        opt.exp_avg, opt.exp_avg_sq = opt.exp_avg[:N], opt.exp_avg_sq[:N]
        if ema:
            opt.ema = opt.ema[:N]
    return flat, opt, keep, base, c


def _one(form, flat, opt, g):
    """One update of ``form`` from gradient ``g``, host and device step numbers kept in step."""
    flat.grad.copy_(g)
    if form == "step":
        opt.step()
        return
    opt.sync_device_step()
    if form == "graphable":
        opt.step_graphable()
    else:
        opt.device_step().add_(1)  # what the caller's step prologue / encoder GEMM does
        if form == "prebumped":
            opt.step_graphable(prebumped=True)
        else:
            opt.step_pack()
    opt.step_count += 1


def _sha(t):
    t = t.detach().reshape(-1).contiguous().cpu().view(torch.uint8)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def run_case(name):
    """``{tensor name: sha256}`` of case ``name``."""
    form, clip, sched, ema, kind = cases()[name]
    flat, opt, keep, base, c = _build(form, clip, sched, ema)
    n = flat.grad.numel()
    clipped = []
    for s, scale in enumerate(SCALES if kind != "prime" else SCALES[:1]):
        g = _randn(n, 100 + s) * (base * scale)
        if kind == "skip" and s == 1:
            g[n // 2] = float("inf")
        _one(form, flat, opt, g.to(DEV))
        if clip:
            clipped.append(float(opt.grad_norm) > c)
    if kind == "prime":
        flat.grad.copy_((_randn(n, 200) * base).to(DEV))
        opt.sync_device_step()
        opt.step_pack(update=False, gofs=0)
    torch.cuda.synchronize()
    if kind == "updates" and clip:
        assert True in clipped and False in clipped, (name, clipped)
    if kind == "skip":
        assert int(opt.skipped_steps) == 1 and math.isfinite(float(opt.grad_norm)), name
    out = {k: _sha(t) for k, t in keep.items()}
    for k in ("applied_lr", "grad_norm", "skipped_steps", "applied_ema_decay"):
        if getattr(opt, k) is not None:
            out[k] = _sha(getattr(opt, k))
    if form != "step":
        out["device_step"] = _sha(opt.device_step())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--record", metavar="PATH")
    ap.add_argument("--commit", help="id of the commit the record is made from")
    ap.add_argument("--only", default=None, help="run this one case and print it (no file)")
    a = ap.parse_args(argv)
    for k in SWITCHES:
        os.environ.pop(k, None)
    if a.only:
        print(json.dumps({a.only: run_case(a.only)}, indent=1))
        return 0
    if not (a.record and a.commit):
        ap.error("--record PATH and --commit ID are required")
    cc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout
    rec = {"commit": a.commit,
           "hipcc": next((l.strip() for l in cc.splitlines() if "clang version" in l), ""),
           "cases": {name: run_case(name) for name in cases()}}
    with open(a.record, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(rec["cases"]), "cases to", a.record)
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main())
