"""Trainer base — the ``COINNTrainer`` role.

A task plugin subclasses :class:`NNTrainer` exactly like the reference's
``FreeSurferTrainer(COINNTrainer)`` (``comps/fs/__init__.py:42-63``): it registers modules in
``self.nn`` from ``_init_nn_model`` and implements ``iteration(batch)`` returning
``{'out', 'loss', 'averages', 'metrics', ...}``.  The base owns device placement, the flat
fp32 parameter buffer + fused Adam (``learning_rate``), evaluation, checkpoints with the
reference ``state_dict`` key names, and the fast training step.

Fast path: a plugin that implements ``forward_loss(x, y) -> (out, loss, pred)`` and
``score(out, pred)`` gets the HIP-graph-captured :class:`runtime.step.TrainStep`; any other
plugin trains through ``iteration`` eagerly (still on the fused kernels).
"""
from __future__ import annotations

import os
import random
from typing import Any, Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from ..config import lr_schedule_of
from ..ops import FlatParams, FusedAdam
from ..utils.metrics import Averages, Metrics


def set_seed(seed: int):
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)


class NNTrainer:
    def __init__(self, cache: Optional[Dict[str, Any]] = None, state: Optional[Dict[str, Any]] = None,
                 device=None, **kw):
        self.cache = cache if cache is not None else {}
        self.state = state if state is not None else {}
        dev = torch.device(device) if device is not None else torch.device("cpu")
        self.device = {"gpu": dev}
        self.nn: Dict[str, nn.Module] = {}
        self.flat: Optional[FlatParams] = None
        self.optimizer: Optional[FusedAdam] = None

    # ---- plugin hooks ------------------------------------------------------------------------
    def _init_nn_model(self):
        raise NotImplementedError

    def iteration(self, batch) -> Dict[str, Any]:
        """Default iteration for plugins that implement ``forward_loss``."""
        x = batch["inputs"].to(self.device["gpu"], non_blocking=True)
        y = batch["labels"].to(self.device["gpu"], non_blocking=True).long()
        out, loss, pred = self.forward_loss(x, y)
        m = self.new_metrics()
        m.add(self.score(out, pred), y)
        a = self.new_averages()
        a.add(loss.detach(), len(x))
        return {"out": out, "loss": loss, "averages": a, "metrics": m, "prediction": pred,
                "indices": batch.get("ix")}

    def forward_loss(self, x, y):  # pragma: no cover - optional fast path
        raise NotImplementedError

    def split_module(self):
        """A model with ``stem`` / ``body_loss`` / ``stem_parameters`` whose
        ``body_loss(stem(x), y)`` equals :meth:`forward_loss` (enables the split-capture
        training step), or None."""
        return None

    def score(self, out, pred):
        return pred

    # the column of ``out`` that :meth:`score` returns, when it is one (a device-fed epoch then
    # records it on the device every step: ``runtime.feed``); None keeps the host-fed loop
    score_column: Optional[int] = None

    @property
    def reference_math(self) -> bool:
        """``compute_path = "reference"``: every model runs the fp32 oracle math
        (``ops/reference.py``) instead of the fused kernels, on whatever device it lives on."""
        return str(self.cache.get("compute_path", "fused")) == "reference"

    @property
    def has_fast_path(self) -> bool:
        return type(self).forward_loss is not NNTrainer.forward_loss

    # ---- loss options (ops.head: class weights / label smoothing) ------------------------------
    def loss_option_args(self) -> Dict[str, Any]:
        """Constructor arguments of the task's model from the cache keys ``class_weights`` /
        ``label_smoothing``.  ``"balanced"`` builds the model with the options on and unit
        weights; the site loop sets the resolved weights before the first step
        (``runtime.site.FederatedSite``, :meth:`set_loss_options`)."""
        cw = self.cache.get("class_weights")
        if isinstance(cw, str):
            if cw != "balanced":
                raise ValueError(f"class_weights {cw!r}: expected a list, 'balanced' or None")
            cw = [1.0] * int(self.cache.get("num_class", 2))
        return {"class_weights": cw, "label_smoothing": self.cache.get("label_smoothing") or 0.0}

    def _head_specs(self):
        return [m.head_spec() for m in self.nn.values() if hasattr(m, "head_spec")]

    def loss_options(self) -> Optional[Dict[str, Any]]:
        """The resolved ``{"class_weights": [...], "label_smoothing": eps}`` the models train
        with, or None when the options are off."""
        for spec in self._head_specs():
            if spec.loss_on:
                w = spec.class_weights or [1.0] * spec.num_class
                return {"class_weights": [float(v) for v in w],
                        "label_smoothing": float(spec.label_smoothing)}
        return None

    def set_loss_options(self, class_weights=None, label_smoothing=None):
        """New values in place (captured graphs follow; raises if the models were built with the
        options off)."""
        for spec in self._head_specs():
            spec.set_loss(class_weights, label_smoothing)

    # ---- framework -----------------------------------------------------------------------------
    def new_metrics(self) -> Metrics:
        return Metrics(int(self.cache.get("num_class", 2)))

    def new_averages(self) -> Averages:
        return Averages()

    def init_nn(self, init_model: bool = True, init_optimizer: bool = True, seed: Optional[int] = None):
        if seed is not None:
            set_seed(seed)
        if init_model:
            self.nn = {}
            self._init_nn_model()
            for k in self.nn:
                self.nn[k] = self.nn[k].to(self.device["gpu"])
            if self.reference_math:
                for net in self.nn.values():
                    for m in net.modules():
                        if hasattr(m, "use_fused"):
                            m.use_fused = False
        if init_optimizer:
            self._init_optimizer()

    def parameters(self):
        for k in sorted(self.nn):
            yield from self.nn[k].parameters()

    def _init_optimizer(self, lr: Optional[float] = None, cache: Optional[Dict[str, Any]] = None):
        """``cache``: the phase's configuration where it differs from the run's (pretraining)."""
        cache = self.cache if cache is None else cache
        self.flat = FlatParams(self.parameters(), device=self.device["gpu"])
        lr = float(lr if lr is not None else cache.get("learning_rate", 1e-3))
        # (0 = off -> None, so the DINUNET_MAX_GRAD_NORM switch still applies; likewise an
        # unset schedule and DINUNET_LR_SCHEDULE, ema_decay and DINUNET_EMA_DECAY)
        ew = cache.get("ema_warmup")
        self.optimizer = FusedAdam(self.flat, lr=lr, weight_decay=float(cache.get("weight_decay", 0.0)),
                                   max_grad_norm=float(cache.get("max_grad_norm") or 0) or None,
                                   lr_schedule=lr_schedule_of(cache),
                                   ema_decay=float(cache.get("ema_decay") or 0) or None,
                                   ema_warmup=True if ew is None else bool(ew))

    def modules(self) -> nn.Module:
        """All registered modules as one container (engines walk ``.modules()``)."""
        return nn.ModuleDict({k: v for k, v in self.nn.items()})

    def train(self):
        for m in self.nn.values():
            m.train()

    def eval(self):
        for m in self.nn.values():
            m.eval()

    def ema_weights(self):
        """The scope an evaluation runs in: the parameters are the optimizer's weight average
        inside it (``FusedAdam.ema_weights``, swapped back when it ends); nothing with the
        average off."""
        opt = self.optimizer
        if opt is not None and getattr(opt, "ema", None) is not None:
            return opt.ema_weights()
        import contextlib
        return contextlib.nullcontext()

    @torch.no_grad()
    def evaluate(self, loader) -> Dict[str, Any]:
        """Run ``iteration`` over a loader; returns merged averages/metrics and predictions."""
        self.eval()
        avg, met = self.new_averages(), self.new_metrics()
        outs = []
        for x, y, ix in loader:
            it = self.iteration({"inputs": x, "labels": y, "ix": ix})
            avg.accumulate(it["averages"])
            met.accumulate(it["metrics"])
            outs.append(it["out"].detach())
        self.train()
        return {"averages": avg, "metrics": met, "out": torch.cat(outs) if outs else None}

    # ---- checkpoints (reference state_dict key names) -------------------------
    def checkpoint_state(self, **extra) -> Dict[str, Any]:
        st = {"models": {k: {n: t.detach().cpu() for n, t in v.state_dict().items()}
                         for k, v in self.nn.items()}}
        if self.optimizer is not None:
            st["optimizer"] = self.optimizer.state_dict()
        lo = self.loss_options()
        if lo is not None:  # beside the model section: a resume / test continues the objective
            st["loss_options"] = lo
        ema = getattr(self.optimizer, "ema", None)
        if ema is not None:
            # the flat average beside the model section (which stays the raw weights under the
            # reference's key names): what validation scored is what a test pass scores
            st["ema"] = ema.detach().cpu()
        st.update(extra)
        return st

    # ---- random state (resume continues the same training curve) -------------
    def rng_state(self) -> Dict[str, Any]:
        """Every generator a training step draws from: torch (CPU, and the device's when on a
        GPU), Python ``random``, NumPy, and the device-side dropout counters of fused heads."""
        npst = np.random.get_state()
        st: Dict[str, Any] = {
            "torch": torch.get_rng_state(),
            "python": random.getstate(),
            "numpy": {"keys": torch.from_numpy(npst[1].astype(np.int64)), "pos": int(npst[2]),
                      "has_gauss": int(npst[3]), "cached": float(npst[4])},
        }
        dev = self.device["gpu"]
        if dev.type == "cuda":
            st["cuda"] = torch.cuda.get_rng_state(dev)
        heads = {}
        for k, m in self.nn.items():
            spec = getattr(m, "_head", None)
            if spec is not None and getattr(spec, "_rng", None) is not None:
                heads[k] = spec._rng.detach().cpu().clone()
        st["heads"] = heads
        return st

    def load_rng_state(self, st: Dict[str, Any]):
        torch.set_rng_state(st["torch"])
        py = st["python"]
        random.setstate((py[0], tuple(py[1]), py[2]))
        n = st["numpy"]
        np.random.set_state(("MT19937", n["keys"].numpy().astype(np.uint32), n["pos"],
                             n["has_gauss"], n["cached"]))
        dev = self.device["gpu"]
        if dev.type == "cuda" and "cuda" in st:
            torch.cuda.set_rng_state(st["cuda"], dev)
        for k, t in (st.get("heads") or {}).items():
            spec = getattr(self.nn.get(k), "head_spec", None)
            if spec is not None:
                spec().rng(dev).copy_(t.to(dev))

    def save_checkpoint(self, path: str, **extra):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + ".tmp"
        torch.save(self.checkpoint_state(**extra), tmp)
        os.replace(tmp, path)

    def load_checkpoint(self, path: str, load_optimizer: bool = False) -> Dict[str, Any]:
        st = torch.load(path, map_location="cpu", weights_only=True)
        self.load_state(st, load_optimizer)
        return st

    def load_state(self, st: Dict[str, Any], load_optimizer: bool = False):
        models = st.get("models", st)
        for k, sd in models.items():
            if k in self.nn:
                self.nn[k].load_state_dict(sd)
        if load_optimizer and self.optimizer is not None and "optimizer" in st:
            self.optimizer.load_state_dict(st["optimizer"])
        lo = st.get("loss_options")
        if lo and self.loss_options() is not None:
            self.set_loss_options(lo["class_weights"], lo["label_smoothing"])
        ema = getattr(self.optimizer, "ema", None)
        if ema is not None:
            # the average as checkpointed, with or without the optimizer's state; a checkpoint
            # that carries none restarts it at the loaded weights
            if st.get("ema") is not None and st["ema"].numel() == ema.numel():
                ema.copy_(st["ema"].to(ema.device))
            elif not (load_optimizer and "ema" in (st.get("optimizer") or {})):
                ema.copy_(self.flat.data)
