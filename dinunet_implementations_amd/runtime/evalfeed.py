"""Device-fed evaluation: a validation / test pass as replays of captured forward-only graphs.

``NNTrainer.evaluate`` walks a loader from the host and runs ``iteration`` eagerly per batch (the
reference's loop, ``comps/icalstm/__init__.py:56-70`` under ``no_grad``).  :class:`EvalFeed` runs
the same pass -- the same batches in the same order, the same kernels on the same rows -- with
the split resident in HBM (bf16 for models that take a bf16 batch, else fp32 rows padded to 8
features) and no host work between batches:

* the batch partition is the unshuffled loader's (:func:`eval_partition`): full batches, then one
  tail batch (``r`` rows; ``batch_size + 1`` when the loader would merge a trailing singleton);
* full batches replay graphs of K batches (``feed.default_graph_steps``), the tail has a graph at
  its exact row count; the graphs are linear;
* a batch is the model's forward (ICA: encoder GEMM, projection GEMM, forward-only recurrence,
  the head's evaluation forward) and ONE boundary launch (``eval.hip``) that files its outputs
  into the pass-level arrays and gathers the next batch.  The packed LSTM / encoder operand
  images are rewritten from the parameters by one launch at the start of every pass, so the
  graphs -- which read parameters and BatchNorm running statistics in place -- stay valid across
  epochs, optimizer steps and checkpoint reloads;
* one device-to-host read per pass; the loss average is accumulated per batch as ``Averages``
  does, the scores are ``trainer.score(out, pred)`` over the whole pass.

The pass writes nothing a training step reads: no gradient, optimizer, cursor or dropout state.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..ops import DeviceSource, _lib
from ..ops.evalpass import EvalPass
from ..ops.lstm import PersistentPack, use_persistent
from ..utils.metrics import Averages
from .feed import default_graph_steps


def eval_partition(n: int, batch_size: int) -> Tuple[int, int]:
    """``(full batches, tail rows)`` of an unshuffled pass over ``n`` samples: the batches of
    ``DeviceLoader(shuffle=False, drop_last=False, merge_singleton=True)``.  ``tail`` is 0, the
    ``n % batch_size`` remaining rows, or ``batch_size + 1`` when a trailing 1-sample batch is
    folded into the batch before it."""
    n, bs = int(n), max(1, int(batch_size))
    if n <= 0:
        return 0, 0
    nb = (n + bs - 1) // bs
    if nb > 1 and n % bs == 1:
        nb -= 1
    tail = n - (nb - 1) * bs
    return (nb, 0) if tail == bs else (nb - 1, tail)


def eval_spans(n: int, batch_size: int) -> List[Tuple[int, int]]:
    """``[(start, end)]`` per batch of :func:`eval_partition`."""
    full, tail = eval_partition(n, batch_size)
    bs = max(1, int(batch_size))
    spans = [(b * bs, (b + 1) * bs) for b in range(full)]
    if tail:
        spans.append((full * bs, full * bs + tail))
    return spans


def resident_bytes(X: torch.Tensor, bf16: bool) -> int:
    """HBM the feed's own copy of ``X`` takes (0 when ``X`` is used in place)."""
    row = X[0].numel() if X.shape[0] else 0
    if bf16:
        return 0 if X.dtype == torch.bfloat16 else X.shape[0] * 2 * row
    if X.dtype == torch.float32 and row % 8 == 0:
        return 0
    return X.shape[0] * 4 * (-(-row // 8) * 8)


class _EvalPack(PersistentPack):
    """The operand images of a ``PersistentPack`` with the fused ``b_ih + b_hh`` bias image of
    ``dn_lstm_pack``, rewritten from the parameters by ONE pack launch (:meth:`refresh`) -- what
    the model's own pack launch produces, without a launch per batch."""

    def __init__(self, pp: PersistentPack):
        self.__dict__.update(pp.__dict__)
        self.extra_src, self.extra = [], []
        self.bias_p = torch.zeros(self.ndir * 4 * self.HD, dtype=torch.float32,
                                  device=self.wih_p.device)

    def refresh(self):
        ps = [p.detach() for p in self.params] + [None] * (8 - len(self.params))
        nc = len(self.cast_src)
        P, I_ = ctypes.c_void_p, ctypes.c_int
        _lib.call("dn_lstm_pack", *[_lib.ptr(p) for p in ps], self.I, self.Hd, self.ndir,
                  self.wih_p.data_ptr(), self.bias_p.data_ptr(), self.whh_p.data_ptr(),
                  self.whhT_p.data_ptr(), nc,
                  (P * max(nc, 1))(*[c.data_ptr() for c in self.cast_src]),
                  (P * max(nc, 1))(*[d.data_ptr() for d in self.casts]),
                  (I_ * max(nc, 1))(*[c.numel() for c in self.cast_src]), _lib.stream())


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class EvalFeed:
    """``EvalFeed(trainer, X, Y, batch_size).run()`` == ``trainer.evaluate(DeviceLoader(X, Y,
    batch_size))``: the dict ``{"averages", "metrics", "out"}`` (plus the pass's ``pred`` and
    per-batch ``losses``).  ``group``: the site's process group (captures on an RCCL group wait
    for its eager collectives first)."""

    def __init__(self, trainer, X: torch.Tensor, Y: torch.Tensor, batch_size: int,
                 steps_per_graph: Optional[int] = None, group=None):
        if not X.is_cuda:
            raise ValueError("EvalFeed: the split must live on the GPU")
        if X.shape[0] < 1:
            raise ValueError("EvalFeed: empty split")
        if not trainer.has_fast_path:
            raise ValueError("EvalFeed: the trainer has no forward_loss")
        self.trainer = trainer
        self.group = group
        self.B = max(1, int(batch_size))
        self.N = int(X.shape[0])
        sm = trainer.split_module()
        if sm is not None and getattr(sm, "accepts_bf16_input", False) and hasattr(sm, "forward_loss"):
            # the model itself on the bf16 batch: trainer.forward_loss would widen it to fp32
            # and the model round it back (two cast launches per batch, the same values)
            self._fwd = sm.forward_loss
            Xr = X if X.dtype == torch.bfloat16 else X.to(torch.bfloat16)
        else:
            sm = None
            self._fwd = trainer.forward_loss
            Xr = X.float()
        self.src = DeviceSource(Xr, Y, 1)
        self.Yh = self.src.Y.cpu()  # labels of the pass, in order (host: the pass's scores are too)
        self.nfull, self.tail = eval_partition(self.N, self.B)
        self.nb = self.nfull + (1 if self.tail else 0)
        self.K = (steps_per_graph or default_graph_steps(self.nfull)) if self.nfull else 0
        C = int(trainer.cache.get("num_class", 2))
        self.ps = EvalPass(self.src, max(self.B if self.nfull else 0, self.tail), self.nb, C)
        self.pack: Optional[_EvalPack] = None
        pp = sm.persistent_pack(X.device) if (sm is not None and hasattr(sm, "persistent_pack")) else None
        if pp is not None:
            self.pack = _EvalPack(pp)
        self._graphs: Dict[Tuple[int, int], torch.cuda.CUDAGraph] = {}
        self._warm: set = set()
        self._sig = None
        self.passes = 0

    # ---- one batch ----------------------------------------------------------------------------
    def _forward(self, rows: int):
        x = self.src.view(self.ps.xb)[:rows]
        y = self.ps.yd[:rows]
        with (use_persistent(self.pack) if self.pack is not None else _Null()):
            out, loss, pred = self._fwd(x, y)
        if self.pack is not None and not self.pack.used:
            raise RuntimeError("EvalFeed: the model's forward did not take the packed operands")
        if out.dtype != torch.float32 or out.stride(1) != 1:
            out = out.float().contiguous()
        if loss.dtype != torch.float32:
            loss = loss.float()
        if pred.dtype != torch.int64 or not pred.is_contiguous():
            pred = pred.long().contiguous()
        if out.shape != (rows, self.ps.C):
            raise RuntimeError(f"EvalFeed: output {tuple(out.shape)}, want {(rows, self.ps.C)}")
        return out, loss, pred

    def _batch(self, rows: int):
        """A batch of ``rows`` rows as issued into the current stream: forward + boundary."""
        out, loss, pred = self._forward(rows)
        self.ps.boundary(out, loss, pred, rows)

    def _check_storage(self):
        """The graphs hold the parameters' addresses: a trainer that re-homed its parameters (a
        new flat buffer, ``NNTrainer._init_optimizer`` after pretraining) gets new graphs."""
        flat = getattr(self.trainer, "flat", None)
        sig = flat.data.data_ptr() if flat is not None else None
        if sig != self._sig:
            self._graphs.clear()
            self._sig = sig

    def _graph(self, rows: int, k: int) -> torch.cuda.CUDAGraph:
        g = self._graphs.get((rows, k))
        if g is None:
            from .step import CAPTURE_MODE, _quiesce_collectives
            if rows not in self._warm:
                # once per row count, eagerly and off the capture stream: lazy initialisation
                # (kernel modules, layout tables) must not happen inside a capture
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self._forward(rows)
                torch.cuda.current_stream().wait_stream(s)
                self._warm.add(rows)
            if self.group is not None:
                _quiesce_collectives(self.group)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                for _ in range(k):
                    self._batch(rows)
            self._graphs[(rows, k)] = g
        return g

    def prepare(self):
        """Capture every graph :meth:`run` replays (so a timed pass holds no capture)."""
        tr = self.trainer
        tr.eval()
        try:
            with torch.no_grad():
                self._check_storage()
                if self.pack is not None:
                    self.pack.refresh()
                for rows, k in self._plan():
                    self._graph(rows, k)
        finally:
            tr.train()

    def _plan(self) -> List[Tuple[int, int]]:
        """``(rows, batches)`` of the graph replays of one pass, in order."""
        plan = []
        if self.nfull:
            plan += [(self.B, self.K)] * (self.nfull // self.K)
            if self.nfull % self.K:
                plan.append((self.B, self.nfull % self.K))
        if self.tail:
            plan.append((self.tail, 1))
        return plan

    # ---- a pass ------------------------------------------------------------------------------
    @torch.no_grad()
    def run(self) -> Dict[str, Any]:
        tr, ps = self.trainer, self.ps
        tr.eval()
        try:
            self._check_storage()
            if self.pack is not None:
                self.pack.refresh()
            graphs = [self._graph(rows, k) for rows, k in self._plan()]
            ps.reset()
            ps.boundary()  # the first batch into the static input
            for g in graphs:
                g.replay()
            host = ps.buf.cpu()  # the pass's one device-to-host read (synchronises)
        finally:
            tr.train()
        self.passes += 1
        out_h, loss_h, pred_h = ps.views(host)
        # sum of fp32(loss_b * n_b) in batch order, as Averages.add / accumulate form it
        total = 0.0
        lb = loss_h.numpy()
        for b, (s, e) in enumerate(eval_spans(self.N, self.B)):
            total += float(np.float32(lb[b]) * np.float32(e - s))
        avg = Averages.from_state({"sum": total, "n": self.N})
        met = tr.new_metrics()
        met.add(tr.score(out_h, pred_h), self.Yh)
        return {"averages": avg, "metrics": met, "out": ps.out_all.clone(),
                "pred": ps.pred_all.clone(), "losses": loss_h.clone()}
