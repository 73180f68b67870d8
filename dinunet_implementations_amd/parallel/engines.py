"""Gradient-aggregation engines: dSGD, rank-dAD, PowerSGD (reference ``comps/__init__.py:13-16``),
top-k sparsification, the coordinate-wise trimmed mean, and federated averaging with local steps.

Each engine turns every site's local gradient (living in the flat grad buffer of
``ops.FlatParams``) into the *global* update all sites apply with their own optimizer, so
replicas stay identical:

* ``dSGD``     mean of site gradients — one (bucketed, backward-overlapped) RCCL all-reduce.
* ``rankDAD``  for every ``nn.Linear``: rank-r factors of ``Delta^T A`` from a structured power
  iteration (``lowrank.dad_factors``), all-gathered (a few KB per layer), reconstructed as
  ``mean_s P_s Q_s^T``; exact dAD (raw ``A``, ``Delta`` exchange) when r covers the full rank.
  Every other parameter (biases, BatchNorm) falls back to the dSGD mean.
* ``powerSGD`` rank-r ``P = M Q`` / ``Q = M^T P`` with two all-reduces, warm-started ``Q`` and
  per-site error feedback (Vogels et al. 2019); vectors use the dSGD mean.
* ``topK``     magnitude top-k sparsification with per-rank error feedback: every rank releases
  the ``k = ceil(topk_ratio * n)`` largest entries of ``gradient + residual`` as (index, value)
  pairs, one all-gather, and every rank sums the pairs in rank order (``ops.topk``).
* ``trimmedMean`` every site's dense gradient is gathered; per coordinate the ``trim_sites``
  smallest and largest of the sites' values are dropped and the rest averaged (the median by
  default), so one site's NaN or blown-up gradient does not reach the update (``ops.trimmed``).
* ``fedAvg``   the one engine that does not exchange at every update: ``fedavg_local_steps``
  one-site updates per site, then one mean of the sites' parameter differences (``ops.fedavg``).

Every engine also exposes the three pieces the COINSTAC file transport needs
(``payload`` on a site, ``aggregate`` on the remote, ``apply`` back on the site) with the same
arithmetic as the collective path (``compat/``).

``reduce()`` returns the scale the optimizer must apply to the flat gradient (dSGD leaves the
all-reduce SUM in place and folds ``1/world`` into the fused Adam launch).
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn

from ..ops import _grad as _gradreg
from ..ops import _lib
from ..ops import capture as _cap
from ..ops.dp import DPState
from ..ops.fedavg import FedAvgState, site_weights
from ..ops.optim import FlatParams
from ..ops.secagg import SecAggState
from ..ops.topk import FLOAT_INDEX_MAX, TopKState
from ..ops.trimmed import MAX_SITES as TRIM_MAX_SITES
from ..ops.trimmed import TrimmedState
from .collective import (PAYLOAD_TYPES, SB, DirectMean, DirectSum, from_payload, launch_on,
                         payload_name, payload_numel, to_payload)
from .group import SiteGroup
from .lowrank import EPS as EPS_MGS
from .lowrank import LowRankTable, PiReconTable, _mgs_torch_, dad_factors, orthonormalize_

Tensor = torch.Tensor


COLLECTIVES = ("auto", "allreduce", "direct", "peer", "calibrate")

DP_STREAM_RANKS = 2048  # ranks per (fold, phase) in the generator's stream word


def dp_options(cfg: dict) -> Tuple[float, float]:
    """``(dp_clip_norm, dp_noise_multiplier)`` of ``cfg``; where a key is unset (None / 0) the
    ``DINUNET_DP_CLIP_NORM`` / ``DINUNET_DP_NOISE`` switch applies.  Clip 0: the option is off."""
    c = float(cfg.get("dp_clip_norm") or os.environ.get("DINUNET_DP_CLIP_NORM", "") or 0)
    s = float(cfg.get("dp_noise_multiplier") or os.environ.get("DINUNET_DP_NOISE", "") or 0)
    if not (0.0 <= c <= 3.4e38) or not (0.0 <= s <= 3.4e38):
        raise ValueError(f"dp_clip_norm / dp_noise_multiplier must be finite numbers >= 0, got "
                         f"{c!r} / {s!r}")
    if s > 0 and not c > 0:
        raise ValueError("dp_noise_multiplier > 0 needs dp_clip_norm > 0 (the noise is scaled by "
                         "the clip threshold)")
    return c, s


def secure_agg_option(cfg: dict) -> bool:
    """Is ``secure_agg`` on in ``cfg``?  Where the key is unset (None / false) the
    ``DINUNET_SECURE_AGG=1`` switch applies."""
    v = cfg.get("secure_agg")
    if v is not None and not isinstance(v, bool):
        raise ValueError(f"secure_agg must be true or false, got {v!r}")
    return bool(v) or os.environ.get("DINUNET_SECURE_AGG", "") == "1"


def topk_ratio_option(cfg: dict) -> float:
    """``topk_ratio`` of ``cfg`` (default 0.01): the share of the gradient's elements a rank
    releases per step, in (0, 1]."""
    v = cfg.get("topk_ratio")
    v = 0.01 if v is None else v
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 < v <= 1):
        raise ValueError(f"topk_ratio must be a number in (0, 1], got {v!r}")
    return float(v)


def trim_sites_option(cfg: dict):
    """``trim_sites`` of ``cfg`` (default ``"median"``): the sites dropped at each end of every
    coordinate's sorted values -- ``"median"`` or an integer >= 0."""
    v = cfg.get("trim_sites")
    v = "median" if v is None else v
    if v == "median" and isinstance(v, str):
        return v
    if (isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 <= v < 2 ** 31)
            or v != int(v)):
        raise ValueError(f"trim_sites must be 'median' or an integer >= 0, got {v!r}")
    return int(v)


_WARNED_TWO_PARTIES = False


class Engine:
    name = "base"
    # does the engine release a gradient (ops.dp can privatise it)?  The low-rank engines share
    # factors / activations instead
    supports_dp = False
    # ... and can ops.secagg mask it?
    supports_secure_agg = False
    # what the engine puts on the wire instead (the refusals of the two options say it)
    releases = "factors, not a gradient"

    def __init__(self, model: nn.Module, flat: FlatParams, group: SiteGroup, cfg: Optional[dict] = None):
        self.model = model
        self.flat = flat
        self.group = group
        self.cfg = dict(cfg or {})
        # wire type of every site-mean (collective.payload_name): fp16 at precision_bits=16 like
        # the reference, or the explicit ``payload_dtype``; always accumulated in fp32
        self.wire = payload_name(self.cfg)
        self.half = self.wire != "fp32"
        self.comm_bytes = 0  # payload bytes this site sent in the last reduce (observability)
        self._means: Dict[Tuple[int, int], DirectMean] = {}
        # ``dsgd_collective``: the site-mean form of every engine -- "allreduce" (RCCL / gloo),
        # "direct" (all-to-all + fp32 sum + all-gather through the process group), "peer" (the
        # IPC-mapped HBM exchange of parallel/peer.py: kernels only, captured in the step's
        # graph on any backend), "auto" (peer for 16-bit wires on GPU sites -- the fp32-sum form
        # the reference's 16-bit payloads need, captured -- else all-reduce), "calibrate"
        # (dSGD: measured; the low-rank engines take auto's choice)
        coll = str(self.cfg.get("dsgd_collective", "auto"))
        if coll not in COLLECTIVES:
            raise ValueError(f"dsgd_collective {coll!r}: expected one of {', '.join(COLLECTIVES)}")
        self.collective = coll
        # secure aggregation (ops.secagg, dSGD only): on / off is fixed here, the device block
        # and the key agreement follow in DSGDEngine
        self.sa: Optional[SecAggState] = None
        self.secure_agg = secure_agg_option(self.cfg)
        if self.secure_agg:
            if not self.supports_secure_agg:
                raise ValueError(f"secure_agg: the masked gradient sum is implemented for dSGD "
                                 f"only ({self.name} shares {self.releases})")
            if self.half:
                raise ValueError(f"secure_agg: the wire is the uint64 fixed-point image of the "
                                 f"fp32 gradient; a {self.wire} payload (precision_bits=16 / "
                                 f"payload_dtype) does not combine with it")
            if coll == "allreduce":
                raise ValueError("secure_agg: dsgd_collective='allreduce' would form the sum in "
                                 "a library's signed arithmetic; use auto, peer or direct")
            if group.world > SecAggState.MAX_PARTIES:
                raise ValueError(f"secure_agg: at most {SecAggState.MAX_PARTIES} parties (sums of "
                                 f"more do not fit int64), got {group.world}")
        self.peer = self._want_peer(coll)
        # differentially private release (ops.dp): on / off is fixed here.  The generator's
        # stream word fold * 4096 + phase * 2048 + global rank (phase 1: pretraining) keeps every
        # (site, fold, phase, release) on a counter of its own; ``dp_fold`` / ``dp_phase`` come
        # from the site loop
        self.dp: Optional[DPState] = None
        c, sigma = dp_options(self.cfg)
        if c > 0:
            if not self.supports_dp:
                raise ValueError(f"dp_clip_norm: the private gradient release is implemented for "
                                 f"dSGD only ({self.name} shares {self.releases})")
            # (``dp_rank``: the global rank of a site that trains alone in a group of its own)
            rank = int(self.cfg.get("dp_rank", group.rank))
            if not (0 <= rank < DP_STREAM_RANKS):
                raise ValueError(f"dp_clip_norm: rank {rank} does not fit the generator's "
                                 f"stream word (< {DP_STREAM_RANKS} ranks)")
            seed = self.cfg.get("dp_seed")
            seed = int(self.cfg.get("seed", 0) or 0) if seed is None else int(seed)
            stream = (int(self.cfg.get("dp_fold", 0)) * 2 * DP_STREAM_RANKS
                      + int(bool(self.cfg.get("dp_phase", 0))) * DP_STREAM_RANKS + rank)
            self.dp = DPState(flat.grad.device, c, sigma, seed, stream)

    def _peer_ok(self) -> bool:
        from . import peer as _peer
        return _peer.available(self.group, self.flat.grad.device)

    def _want_peer(self, coll: str) -> bool:
        if not self.group.distributed:
            return False
        if coll == "peer":
            if not self._peer_ok():
                raise ValueError("dsgd_collective='peer' needs GPU sites and the kernel library "
                                 f"(at most 16 sites); device {self.flat.grad.device}")
            return True
        return (coll in ("auto", "calibrate")
                and (self.half or (self.secure_agg and self.group.world > 1)) and self._peer_ok())

    # collective path -------------------------------------------------------------------------
    @property
    def capturable(self) -> bool:
        """Can the step capture this engine's collectives in its HIP graph
        (``runtime.step.TrainStep.comm_graph``)?  Always with the peer exchange (its kernels are
        ordinary launches on the step's stream, whatever the process group); with RCCL for the
        fp32 all-reduce; not for host collectives (gloo) nor for RCCL's all-to-all exchange
        (captured from the exchange's own stream it crashed at capture end,
        ``tools/diag/capture_collectives.py`` a2a_side, RCCL 2.26.6)."""
        if not self.group.distributed or self.peer:
            return True
        return self.group.backend == "nccl" and not self.half

    @property
    def pre_capturable(self) -> bool:
        """May the step capture :meth:`pre_reduce` (the local factorisation) in its graph?  Not
        when it starts with a collective of its own (rank-dAD's site mean over several GPUs per
        site, a host-issued collective on gloo): the step then runs it after the replay."""
        return True

    def _peer_mean(self, tag, n: int):
        from . import peer as _peer
        return _peer.mean(self.group, self.flat.grad.device, n, self.wire, (self.name,) + tuple(tag))

    def step_context(self):
        return contextlib.nullcontext()

    def reduce(self) -> float:
        raise NotImplementedError

    # resume ------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        """Engine state a resumed run needs to continue the same curve (warm-started factors,
        error feedback); empty for stateless engines."""
        return {}

    def load_state_dict(self, sd: Dict[str, object]):
        pass

    # file-transport path (COINSTAC compat) ---------------------------------------------------
    def payload(self) -> Dict[str, Tensor]:
        raise NotImplementedError

    @classmethod
    def aggregate(cls, payloads: Sequence[Dict[str, Tensor]], cfg: Optional[dict] = None) -> Dict[str, Tensor]:
        raise NotImplementedError

    def apply(self, agg: Dict[str, Tensor]) -> float:
        raise NotImplementedError

    # helpers ---------------------------------------------------------------------------------
    def _direct(self, key, n: int, device) -> DirectMean:
        dm = self._means.get(key)
        if dm is None or dm.n != n:
            dm = self._means[key] = DirectMean(self.group, n, self.wire, device)
        return dm

    def _allreduce_mean_(self, buf: Tensor, tag=("mean",)):
        """In-place mean over sites, honouring ``precision_bits`` / ``payload_dtype``: the peer
        exchange when selected (``tag`` names the exchange region: exchanges that may be in
        flight together need their own), else a 16-bit payload goes through the direct exchange
        (fp32 accumulation, collective.DirectMean) and fp32 through the all-reduce."""
        g = self.group
        if not g.distributed:
            return
        if self.peer:
            self.comm_bytes += self._peer_mean(tag, buf.numel()).run_(buf)
        elif self.half:
            self.comm_bytes += self._direct(("mean", buf.numel()), buf.numel(), buf.device).run_(buf)
        else:
            g.all_reduce(buf)
            buf.mul_(1.0 / g.world)
            self.comm_bytes += buf.numel() * 4


class _PeerWork:
    """``Work``-like handle of a pushed peer exchange: ``wait()`` issues its reduce + unpack on
    the current stream."""

    def __init__(self, pm, view: Tensor, scale: float = 1.0):
        self.pm, self.view, self.scale = pm, view, scale

    def wait(self):
        self.pm.finish(self.view, self.scale)


# =============================================================================================
# dSGD
# =============================================================================================
class DSGDEngine(Engine):
    """Bucketed all-reduce of the flat gradient, overlapped with the backward pass.

    Buckets are contiguous ranges of the flat buffer formed in REVERSE parameter order (the
    order gradients become ready: classifier, then LSTM, then encoder for ICA).  A bucket's
    all-reduce is launched from the post-accumulate-grad hook of its last parameter, on RCCL's
    own stream, while autograd keeps computing earlier layers.
    """
    name = "dSGD"
    supports_dp = True
    supports_secure_agg = True

    def __init__(self, model, flat, group, cfg=None, bucket_mb: Optional[float] = None,
                 overlap: bool = True):
        super().__init__(model, flat, group, cfg)
        self.overlap = overlap and group.distributed and bool(self.cfg.get("dsgd_overlap", True))
        self.sync_enabled = True
        if bucket_mb is None:
            bucket_mb = float(self.cfg.get("dsgd_bucket_mb", 4.0))
        cap = int(bucket_mb * (1 << 20) / 4)
        self.buckets: List[Tuple[int, int]] = []
        self._param_bucket: Dict[int, int] = {}
        cur_end, cur_start = None, None
        segs = list(flat.segments())
        for p, o, n in reversed(segs):
            end = o + ((n + 3) // 4) * 4
            if cur_end is None:
                cur_end, cur_start = end, o
            elif cur_end - o > cap and cur_end - cur_start > 0:
                self.buckets.append((cur_start, cur_end))
                cur_end, cur_start = cur_start, o
            else:
                cur_start = o
            self._param_bucket[id(p)] = len(self.buckets)
        if cur_end is not None:
            self.buckets.append((cur_start, cur_end))
        self._pending = [0] * len(self.buckets)
        self._expected = [0] * len(self.buckets)
        for p, _, _ in segs:
            self._expected[self._param_bucket[id(p)]] += 1
        self._handles: Dict[int, object] = {}
        self._half_bufs: Dict[int, Tensor] = {}
        # ``dsgd_collective``: "peer" = the IPC-mapped HBM exchange (peer.py: push / fp32 sum /
        # push back, captured in the step graph); "direct" = all_to_all + fp32 sum + all_gather
        # (collective.py) on a comm stream of its own; "allreduce" = one RCCL all-reduce per
        # bucket (a 16-bit payload is then SUMMED in 16 bits inside RCCL); "auto" = peer for
        # 16-bit payloads on GPU sites (direct off the GPU), all-reduce for fp32; "calibrate" =
        # whichever captured form measures faster on this job's buckets and links
        coll = self.collective
        self.calibration: Optional[dict] = None
        sa_on = self.secure_agg and group.world > 1  # (one party: nothing leaves, no masks)
        if coll == "calibrate" and sa_on:
            coll = "peer" if self.peer else "direct"
            self.calibration = {"choice": coll, "reason": "secure_agg: one captured form (the "
                                "uint64 peer exchange), nothing to time"}
        elif coll == "calibrate":
            coll = self._calibrate()
            self.peer = coll == "peer"
        self.direct = (not self.peer) and (coll == "direct" or (coll == "auto" and self.half)
                                           or sa_on)
        if self.half and not self.direct and not self.peer and self.wire == "fp16":
            # RCCL sums an all-reduce buffer in its own type: unscaled fp16 would flush
            # gradients below ~6e-8 and overflow past 65504 in the sum over sites, and a
            # per-site block scale cannot be summed.  The 16-bit all-reduce therefore ships
            # bf16 (fp32's range); the fp16 wire needs the direct exchange (fp32 sum).
            import warnings
            warnings.warn("dsgd_collective='allreduce' with an fp16 payload: sending bf16 "
                          "(RCCL would sum unscaled fp16); use dsgd_collective='direct' for an "
                          "fp16 wire", RuntimeWarning, stacklevel=2)
            self.wire = "bf16"
        self._comm_stream = (torch.cuda.Stream(device=flat.grad.device)
                             if self.direct and group.distributed and flat.grad.is_cuda else None)
        # the peer exchange takes the whole gradient as ONE exchange after the backward, and the
        # step keeps its backward in one piece (``prefers_split``, runtime.step): the split's
        # extra launches (a second grouped weight-gradient launch and split-K reduce, ~15 us) and a
        # second exchange's three launches cost more than pushing the body bucket early hides
        # (loopback fp16 step: profiles/r6_peer_unsplit_ab.jsonl).  The RCCL all-reduce keeps the
        # split: its buckets run on RCCL's own stream, truly under the encoder backward.
        self.prefers_split = not self.peer
        if self.peer and len(self.buckets) > 1 and bool(self.cfg.get("peer_one_bucket", True)):
            self._set_buckets([(self.buckets[-1][0], self.buckets[0][1])])
        if sa_on:
            self._secagg_build()
        self._peer_build()
        self._hooks = []
        self._delivered = set()
        self.early_launches = 0  # buckets started before reduce() (observability)
        self._in_reduce = False
        if self.dp is not None or self.sa is not None:
            # nothing leaves the site before reduce() has privatised / masked the gradient: no
            # hook-issued launches, no split for the sake of an early bucket, and launch_bucket
            # only records readiness (as the peer path already behaves)
            self.overlap = False
            self.prefers_split = False
        if self.peer:
            # no pushes from autograd's gradient hooks: they run in the autograd thread, on a
            # stream that need not be the step's, and the peer exchange reuses its slots safely
            # only when every push is stream-ordered after the previous exchange's finish
            # (replicas diverged with hook-issued pushes in eager side-stream steps).  The
            # captured step pushes the body bucket between its backward parts itself
            # (launch_bucket); eager steps push every bucket in reduce().
            self.overlap = False
        if self.overlap:
            # autograd fires a parameter's post-accumulate hook even when its producer returned
            # no gradient for it -- which is what the fused ops do: they accumulate into .grad
            # themselves, possibly later (deferred grouped GEMM at the end of the backward), and
            # notify through ops._grad.  A tensor hook sees whether a real gradient arrived, and
            # only then does the post-accumulate hook count the parameter as ready.
            for p, _, _ in segs:
                self._hooks.append(p.register_hook(self._marker(id(p))))
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_accumulated))
            _gradreg.register(self._on_grad)  # fused ops write .grad directly and notify
        self._reset()

    @property
    def capturable(self) -> bool:
        # the peer exchange always; RCCL all-reduce buckets (fp32, or the 16-bit all-reduce)
        if not self.group.distributed or self.peer:
            return True
        return self.group.backend == "nccl" and not self.direct

    def _secagg_build(self):
        """The masked release of the whole gradient as ONE exchange: the key agreement (one
        all-gather of public keys over the process group, ``parallel.secagg``), the device block
        and the wire buffer.  Every rank is a party (a site's replicas count separately)."""
        global _WARNED_TWO_PARTIES
        from . import secagg as _keys
        g, grad = self.group, self.flat.grad
        if grad.numel() % 4:
            raise ValueError("secure_agg: the flat gradient must hold a multiple of 4 elements")
        if g.world == 2 and not _WARNED_TWO_PARTIES:
            import warnings
            _WARNED_TWO_PARTIES = True
            warnings.warn("secure_agg with 2 parties: the sum reveals the peer's gradient to "
                          "each of them (own + peer = sum)", RuntimeWarning, stacklevel=3)
        fold, phase = int(self.cfg.get("dp_fold", 0)), int(bool(self.cfg.get("dp_phase", 0)))
        keys = _keys.agree(g, fold, phase)
        from ..ops import reference as _ref
        self.sa = SecAggState(grad.device, g.world, g.rank, keys, _ref.secagg_domain(fold, phase))
        del keys
        self._sa_wire = self.sa.wire_like(grad)
        self._sa_sum: Optional[DirectSum] = None
        self.sa_transport = "peer" if self.peer else "direct"
        self.sa_logged = 0  # saturated count already reported per epoch (runtime.site)
        self._set_buckets([(0, self.flat.numel)])

    def _calibrate(self) -> str:
        """``dsgd_collective="calibrate"``: time the site-mean forms the step can run on THIS
        job's buckets and links and keep the faster -- the choice the link model of
        ``profiles/r4_comm_model.md`` could only predict (per-hop latency and link rates).

        Each candidate is timed in the form the step will run it: the bucket sequence captured
        in a HIP graph and replayed (``TrainStep.comm_graph`` captures the collectives into the
        step), except an all-reduce over a host backend (gloo), which the step issues from the
        host and which is timed so.  Candidates: the all-reduce and the peer exchange
        (``parallel.peer``, GPU sites).  Only forms with the SAME arithmetic compete: a 16-bit
        wire takes the fp32-sum exchange without a race (peer on GPU sites, else direct) --
        RCCL's all-reduce would sum 16-bit partials, so a timing could change the training
        numerics.  The per-form times are max-reduced over the sites, so every site takes the
        same decision from the same numbers; the record lands in ``self.calibration``
        (``logs.json`` ``dsgd_collective``).  ``dsgd_calibrate_reps`` (default 10) timed
        replays."""
        import time as _time
        g = self.group
        sizes = [e - s for s, e in self.buckets]
        if not g.distributed:
            self.calibration = {"choice": "allreduce", "reason": "one site: no collective"}
            return "allreduce"
        peer_ok = self._peer_ok()
        dev = self.flat.grad.device
        cuda = dev.type == "cuda"
        reps = max(1, int(self.cfg.get("dsgd_calibrate_reps", 10)))
        sync = torch.cuda.synchronize if cuda else (lambda: None)
        bufs = [torch.zeros(n, dtype=torch.float32, device=dev) for n in sizes]
        if self.half:
            note = None
            if peer_ok:
                prange = [(self.buckets[-1][0], self.buckets[0][1])]
                peer_ok, note = self._peer_verify(
                    [torch.zeros(prange[0][1] - prange[0][0], dtype=torch.float32, device=dev)],
                    prange)
            choice = "peer" if peer_ok else "direct"
            self.calibration = {"choice": choice, "wire": self.wire,
                                "reason": "16-bit wire: only the exchange sums in fp32"
                                          + (f"; peer {note}" if note else "")}
            return choice

        def allreduce():
            for b in bufs:
                g.all_reduce(b)

        # the peer exchange as the step would run it: ONE exchange of the whole gradient
        prange = [(self.buckets[-1][0], self.buckets[0][1])]
        pbufs = [torch.zeros(prange[0][1] - prange[0][0], dtype=torch.float32, device=dev)]

        def peer():
            for (s, e), b in zip(prange, pbufs):
                self._peer_mean(("bucket", s, e), e - s).run_(b)

        def host_timed(fn):
            for _ in range(2):
                fn()
            sync()
            g.barrier()
            t0 = _time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            return (_time.perf_counter() - t0) / reps * 1e6

        def graph_timed(fn):
            fn()  # eager once (RCCL communicator / peer regions set up outside the capture)
            from ..runtime.step import _quiesce_collectives
            _quiesce_collectives(g)  # every eager collective retired by the watchdog first
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                fn()
            gr.replay()
            sync()
            g.barrier()
            t0 = _time.perf_counter()
            for _ in range(reps):
                gr.replay()
            sync()
            t = (_time.perf_counter() - t0) / reps * 1e6
            g.barrier()
            del gr
            return t

        rccl_graph = cuda and g.backend == "nccl"
        peer_note = None
        if peer_ok:
            peer_ok, peer_note = self._peer_verify(pbufs, prange)
        times = [graph_timed(allreduce) if rccl_graph else host_timed(allreduce),
                 graph_timed(peer) if peer_ok else float("inf")]
        t = torch.tensor(times, dtype=torch.float64, device=dev if g.backend == "nccl" else "cpu")
        g.all_reduce(t, op=dist.ReduceOp.MAX)
        t_ar, t_peer = (float(v) for v in t.cpu())
        choice = "peer" if t_peer < t_ar else "allreduce"
        self.calibration = {"choice": choice, "allreduce_us": round(t_ar, 2),
                            "peer_us": round(t_peer, 2) if peer_ok else None,
                            "allreduce_form": "captured" if rccl_graph else "host-issued",
                            "peer_form": "captured" if peer_ok else (peer_note or "unavailable"),
                            "bucket_elems": sizes, "sites": g.world, "reps": reps,
                            "wire": self.wire}
        return choice

    def _peer_verify(self, bufs, ranges) -> Tuple[bool, Optional[str]]:
        """Before the peer exchange may compete in ``calibrate``: run it once on every bucket with
        known values (site r sends (r + 1) * v, v small integers: every sum exact) under a short
        wait limit and check the mean and the error words on EVERY site -- a machine whose IPC
        mapping or cross-GPU flags misbehave keeps the all-reduce instead of training on a broken
        exchange.  Returns (usable, reason when not)."""
        from . import peer as _peer
        g = self.group
        note = None
        ok = True
        _lib.call("dn_peer_set_timeout_ms", 2000)
        try:
            for (s, e), b in zip(ranges, bufs):
                v = (torch.arange(e - s, device=b.device, dtype=torch.float32) % 7) + 1.0
                b.copy_(v * float(g.rank + 1))
                self._peer_mean(("bucket", s, e), e - s).run_(b)
            torch.cuda.synchronize()
            want = (g.world + 1) / 2.0
            for (s, e), b in zip(ranges, bufs):
                v = (torch.arange(e - s, device=b.device, dtype=torch.float32) % 7) + 1.0
                if not torch.allclose(b, v * want, rtol=1e-6, atol=0):
                    ok, note = False, "failed verification (wrong mean)"
            errs = _peer.errors()
            if errs:
                ok, note = False, f"failed verification (wait timed out: {errs[0][2]})"
        except RuntimeError as ex:  # e.g. the IPC mapping refused
            ok, note = False, f"failed verification ({type(ex).__name__}: {ex})"[:200]
        finally:
            ms = os.environ.get("DINUNET_PEER_TIMEOUT_MS")
            _lib.call("dn_peer_set_timeout_ms", int(ms) if ms else -1)
        flag = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64,
                            device=self.flat.grad.device if g.backend == "nccl" else "cpu")
        g.all_reduce(flag, op=dist.ReduceOp.MIN)  # one site's failure disqualifies it everywhere
        if flag.item() < 0.5 and ok:
            ok, note = False, "failed verification on another site"
        for b in bufs:
            b.zero_()
        return ok, note

    def _marker(self, pid: int):
        def hook(g):
            if g is not None:
                self._delivered.add(pid)
        return hook

    def _on_accumulated(self, p):
        if id(p) in self._delivered:
            self._delivered.discard(id(p))
            self._on_grad(p)

    def _reset(self):
        self._pending = list(self._expected)
        self._handles.clear()
        self._ready = [False] * len(self.buckets)
        self._next = 0
        self._seen = set()

    def _drain(self):
        """Launch ready buckets strictly in bucket order.  Every rank then issues the same
        collective sequence whatever path produced its gradients: an eager step (autograd hooks,
        e.g. a ragged last batch), a graph replay (``launch_bucket`` / ``reduce``), or a split
        replay.  Out-of-order launches across ranks would pair different buckets in RCCL."""
        while self._next < len(self.buckets) and self._ready[self._next]:
            if self._next not in self._handles:
                self._launch(self._next)
            self._next += 1

    def split_buckets(self, stem_params) -> List[int]:
        """Re-bucket for a step whose backward is replayed in two parts (``TrainStep`` split
        capture): every gradient outside ``stem_params`` first (ready when the first part ends),
        then the stem's.  Returns the bucket ids of the first group; the caller launches them
        with :meth:`launch_bucket` between the two parts, ``reduce()`` launches the rest."""
        ids = {id(p) for p in stem_params}
        segs = list(self.flat.segments())
        stem = [(o, o + ((n + 3) // 4) * 4) for p, o, n in segs if id(p) in ids]
        if not stem:
            raise ValueError("stem parameters are not in the flat buffer")
        s0, s1 = min(a for a, _ in stem), max(b for _, b in stem)
        if sum(b - a for a, b in stem) != s1 - s0 or any(s0 <= o < s1 and id(p) not in ids
                                                        for p, o, _ in segs):
            raise ValueError("stem parameters must occupy one contiguous flat range")
        body = [r for r in ((s1, self.flat.numel), (0, s0)) if r[1] > r[0]]
        self._set_buckets(body + [(s0, s1)])
        self._peer_build()
        return list(range(len(body)))

    def _set_buckets(self, ranges):
        """New contiguous bucket ranges (covering every parameter); per-parameter bookkeeping
        rebuilt to match."""
        segs = list(self.flat.segments())
        self.buckets = list(ranges)
        self._param_bucket = {}
        for p, o, _ in segs:
            self._param_bucket[id(p)] = next(i for i, (a, b) in enumerate(self.buckets) if a <= o < b)
        self._expected = [0] * len(self.buckets)
        for p, _, _ in segs:
            self._expected[self._param_bucket[id(p)]] += 1
        self._half_bufs.clear()
        self._reset()

    def _peer_build(self):
        """The peer exchange of every bucket, built now (arena regions and the IPC handle
        exchange are host work, never inside a capture; every site builds in the same order)."""
        if self.peer and self.sa is not None:
            self._sa_peer()
        elif self.peer:
            for s, e in self.buckets:
                self._peer_mean(("bucket", s, e), e - s)

    def _sa_peer(self):
        from . import peer as _peer
        return _peer.mean(self.group, self.flat.grad.device, self._sa_wire.numel(), _peer.U64,
                          (self.name, "secagg"))

    def launch_bucket(self, b: int):
        """Mark bucket ``b`` ready and start every ready bucket up to it, in order (RCCL stream
        ordered after the current stream)."""
        if self.group.distributed:
            self._ready[b] = True
            if self.dp is None and self.sa is None:  # (else the exchange starts in reduce())
                self._drain()

    def _launch(self, b: int):
        if not self._in_reduce:
            self.early_launches += 1
        if not self._handles:  # first bucket of this step
            self.comm_bytes = 0
        s, e = self.buckets[b]
        view = self.flat.grad[s:e]
        if self.peer:
            # push now (no wait: the peers' data travel under the rest of the backward), reduce
            # + unpack when reduce() waits, in bucket order
            pm = self._peer_mean(("bucket", s, e), e - s)
            pm.start(view)
            self._handles[b] = _PeerWork(pm, view)
            self.comm_bytes += pm.bytes_sent
        elif self.direct:
            dm = self._direct((s, e), e - s, view.device)
            self._handles[b] = launch_on(self._comm_stream, lambda: dm.run_(view))
            self.comm_bytes += dm.n * dm.send.element_size()
        elif self.half:
            buf = self._half_bufs.get(b)
            if buf is None:
                dt = PAYLOAD_TYPES[self.wire][1]  # one unscaled block: headers sum to 0
                buf = self._half_bufs[b] = torch.zeros(payload_numel(e - s), dtype=dt,
                                                       device=view.device)
            to_payload(view, buf, 1, -(-(e - s) // SB) * SB)
            self._handles[b] = self.group.all_reduce(buf, async_op=True)
            self.comm_bytes += (e - s) * buf.element_size()
        else:
            self._handles[b] = self.group.all_reduce(view, async_op=True)
            self.comm_bytes += view.numel() * 4

    def _on_grad(self, p):
        if not self.sync_enabled:
            return
        b = self._param_bucket.get(id(p))
        if b is None or id(p) in self._seen:  # each parameter counts once per step
            return
        self._seen.add(id(p))
        self._pending[b] -= 1
        if self._pending[b] == 0:
            self._ready[b] = True
            self._drain()

    def reduce(self) -> float:
        g = self.group
        if self.dp is not None:  # before any byte of the gradient leaves (one site too)
            self.dp.privatize_(self.flat.grad)
        if not g.distributed:
            self._reset()
            return 1.0
        if self.sa is not None:
            return self._secagg_reduce()
        self._ready = [True] * len(self.buckets)
        self._in_reduce = True
        try:
            self._drain()
        finally:
            self._in_reduce = False
        if self.peer:  # every pushed bucket's reduce + unpack, in bucket order, fused launches
            from . import peer as _peer
            _peer.finish_many([(h.pm, h.view, h.scale) for h in self._handles.values()])
            self._handles.clear()
        for b, h in self._handles.items():
            h.wait()
            if self.half and not self.direct and not self.peer:
                s, e = self.buckets[b]
                buf = self._half_bufs[b]
                from_payload(buf, self.flat.grad[s:e])
        self._reset()
        # the exchanges leave the mean, the all-reduce the sum
        self.last_scale = 1.0 if (self.direct or self.peer) else 1.0 / g.world
        return self.last_scale

    def _secagg_reduce(self) -> float:
        """Mask (after the private release, if any), exchange the uint64 wire -- the peer
        exchange's wrap-around sum, or the host-issued integer direct exchange -- and open: the
        flat gradient then holds the mean, bit-identical on every party."""
        grad, wire = self.flat.grad, self._sa_wire
        self.sa.mask_(grad, wire)
        if self.peer:
            self.comm_bytes = self._sa_peer().run_(wire)
        else:
            if self._sa_sum is None:
                self._sa_sum = DirectSum(self.group, wire.numel(), wire.device)
            self.comm_bytes = self._sa_sum.run_(wire)
        self.sa.open_(wire, grad)
        self._reset()
        self.last_scale = 1.0
        return 1.0

    def close(self):
        for h in self._hooks:
            h.remove()
        self._hooks.clear()
        _gradreg.unregister(self._on_grad)

    def state_dict(self):
        sd = {} if self.dp is None else {"dp": self.dp.state_dict()}
        if self.sa is not None:  # the release number and the counts; never a key
            sd["secure_agg"] = self.sa.state_dict()
        return sd

    def load_state_dict(self, sd):
        if self.dp is not None and sd.get("dp"):
            self.dp.load_state_dict(sd["dp"])
        if self.sa is not None and sd.get("secure_agg"):
            self.sa.load_state_dict(sd["secure_agg"])
            self.sa_logged = int(sd["secure_agg"].get("saturated", 0))

    # file transport
    def payload(self):
        if self.dp is not None:  # (compat/nodes.py refuses the option before it gets here)
            raise RuntimeError("dSGD payload(): the private gradient release runs in reduce(); "
                               "the file transport would ship the gradient as computed")
        if self.secure_agg:  # (compat/nodes.py refuses the option before it gets here)
            raise RuntimeError("dSGD payload(): secure_agg masks the gradient in reduce(); the "
                               "file transport would ship it in the clear")
        g = self.flat.grad
        return {"grad": g.to(PAYLOAD_TYPES[self.wire][1]) if self.half else g.clone()}

    @classmethod
    def aggregate(cls, payloads, cfg=None):
        acc = None
        for p in payloads:
            v = p["grad"].float()
            acc = v.clone() if acc is None else acc.add_(v)
        return {"grad": acc / len(payloads)}

    def apply(self, agg):
        self.flat.grad.copy_(agg["grad"].to(self.flat.grad.device, torch.float32))
        return 1.0


# =============================================================================================
# rank-dAD
# =============================================================================================
class RankDADEngine(Engine):
    name = "rankDAD"

    def __init__(self, model, flat, group, cfg=None):
        super().__init__(model, flat, group, cfg)
        self.rank = int(self.cfg.get("dad_reduction_rank", 10))
        self.iters = int(self.cfg.get("dad_num_pow_iters", 5))
        self.tol = float(self.cfg.get("dad_tol", 1e-3))
        self.linears: List[nn.Linear] = [m for m in model.modules() if isinstance(m, nn.Linear)]
        self._weight_ids = {id(m.weight) for m in self.linears}
        self.dense_segs = [(o, n) for p, o, n in flat.segments() if id(p) not in self._weight_ids]
        self._cap: Optional[_cap.DADCapture] = None
        self._gen = None
        # GPU: factorise in GRADIENT space.  The fused kernels already produce each site's
        # G_s = Delta_s^T A_s in the flat grad buffer, and the structured iteration
        # P <- orth(Delta^T (A Q)), Q <- A^T (Delta P) is exactly the power iteration on G_s:
        # running it on G_s ([out, in], a few hundred KB) instead of the [B*S, .] activation /
        # delta factors gives the same factors without capturing them, with no host sync (the
        # dad_tol early stop is a device-side mask), so it is captured in the step's HIP graph.
        self.fast = bool(flat.data.is_cuda and self.cfg.get("dad_gradient_space", True))
        # the one-launch power iteration spins on per-layer barriers, so all of a launch's
        # workgroups must be resident together: never when several site processes share one GPU
        # (the gloo rehearsal), whose persistent launches could then hold each other's CUs
        shared = getattr(group, "gpu_shared", None)
        if shared is None:  # a group built by hand: assume sharing when ranks outnumber GPUs
            shared = group.distributed and group.world > max(1, torch.cuda.device_count())
        self._persist_ok = bool(self.fast and not shared)
        if self.fast:
            self._init_fast()

    # ---- gradient-space path ---------------------------------------------------------------
    @property
    def pre_capturable(self) -> bool:
        return self.group.replicas <= 1

    @property
    def capturable(self) -> bool:
        # the site mean of several GPUs per site runs in reduce(), outside the graph
        return self.group.replicas <= 1 and Engine.capturable.fget(self)

    def _init_fast(self):
        """Device tables of the factorisation kernels (csrc/kernels/lowrank.hip): per large
        Linear, its gradient view, the warm-start / candidate Q, and the P and Q slots of the
        send buffer that the factor all-gather ships."""
        segs = {id(p): o for p, o, _ in self.flat.segments()}
        dev = self.flat.data.device
        gen = torch.Generator(device="cpu").manual_seed(int(self.cfg.get("seed", 0)) + 777)
        r = max(1, min(self.rank, 16))
        self.fast_layers = []  # (module, flat offset, out, in, r, send offset of P, of Q)
        off = 0
        for m in self.linears:
            out_f, in_f = m.weight.shape
            if self.rank >= min(out_f, in_f):
                continue  # exact mode: the dense mean of G (== sum_s Delta_s^T A_s / W)
            self.fast_layers.append((m, segs[id(m.weight)], out_f, in_f, r, off, off + out_f * r))
            off += (out_f + in_f) * r
        low = {id(l[0].weight) for l in self.fast_layers}
        self.fast_dense = [(o, n) for p, o, n in self.flat.segments() if id(p) not in low]
        # the dense (dSGD-mean) part: adjacent segments merged; one index gather / scatter when
        # they are not one range (no per-segment copies)
        merged: List[List[int]] = []
        for o, n in sorted(self.fast_dense):
            if merged and merged[-1][1] == o:
                merged[-1][1] = o + n
            else:
                merged.append([o, o + n])
        self._dense_ranges = [(a, b) for a, b in merged]
        self._dense_idx = (torch.cat([torch.arange(a, b) for a, b in self._dense_ranges]).to(dev)
                           if len(self._dense_ranges) > 1 else None)
        self._dense_buf = (torch.empty(self._dense_idx.numel(), dtype=torch.float32, device=dev)
                           if self._dense_idx is not None else None)
        # the send slot is also the per-rank stride of the gather: 16-byte multiple, whole payload
        # sub-blocks when the factors travel in 16 bits
        pad = SB if (self.half and self.group.distributed) else 8
        self._send = torch.zeros(-(-max(off, 1) // pad) * pad, dtype=torch.float32, device=dev)
        n = len(self.fast_layers)
        if not n:
            return
        W = self.group.world
        self._gathered = (torch.zeros(W * self._send.numel(), dtype=torch.float32, device=dev)
                          if self.group.distributed else self._send)
        if self.half and self.group.distributed:
            dt = PAYLOAD_TYPES[self.wire][1]
            self._send16 = torch.zeros(payload_numel(self._send.numel()), dtype=dt, device=dev)
            self._gathered16 = torch.zeros(W * self._send16.numel(), dtype=dt, device=dev)
        layers = []
        self._praw = []
        for _, o, out_f, in_f, rr, po, qo in self.fast_layers:
            q = torch.randn(in_f, rr, generator=gen)  # identical on every site (same seed)
            _mgs_torch_(q)
            qsend = self._send[qo:qo + in_f * rr].view(in_f, rr)
            qsend.copy_(q.to(dev))  # the send slot doubles as the next step's warm start
            praw = torch.empty(out_f, rr, dtype=torch.float32, device=dev)
            self._praw.append(praw)
            G = self.flat.grad[o:o + out_f * in_f].view(out_f, in_f)
            layers.append((G, None, praw, self._send[po:po + out_f * rr].view(out_f, rr), qsend))
        self._table = LowRankTable(layers, dev)
        if self.peer:  # the exchanges, built outside any capture (peer.PeerArena)
            from . import peer as _peer
            if self._dense_ranges:
                self._peer_mean(("dense",), sum(b - a for a, b in self._dense_ranges))
            _peer.gather(self.group, dev, self._send.numel(), self.wire, ("rankDAD", "factors"))

        G0, gat0 = self.flat.grad.data_ptr(), self._gathered.data_ptr()
        self._recon = PiReconTable(
            [(G0 + 4 * o, gat0 + 4 * po, gat0 + 4 * qo, out_f, in_f, rr)
             for _, o, out_f, in_f, rr, po, qo in self.fast_layers], dev)

    def state_dict(self):
        if self.fast and getattr(self, "fast_layers", None):
            return {"send": self._send.detach().cpu().clone()}  # holds every warm-start Q
        return {}

    def load_state_dict(self, sd):
        if "send" in sd and getattr(self, "fast_layers", None):
            self._send.copy_(sd["send"].to(self._send.device))

    def pre_reduce(self):
        """Local rank-r factors of every large Linear's gradient into the send buffer: two
        launches per power iteration for all layers (``G Q``; fp64-Gram Cholesky QR + ``G^T P``), the
        ``dad_tol`` stop decided on the device: no host sync, HIP-graph capturable."""
        if not self.fast or not self.fast_layers:
            return
        # several GPUs per site: the site's gradient (mean over its replicas) is what the site
        # factorises; its replicas then compute identical factors
        self.group.site_mean_(self.flat.grad)
        self._dense_start()  # (peer) the dense part travels under the power iteration
        if self._persist_ok and self._table.persist(max(1, self.iters), self.tol):
            return  # every iteration in one launch (lr_persist_kernel)
        for it in range(max(1, self.iters)):
            self._table.gq(it, self.tol)
            self._table.orth_gtp(it)

    def _dense_view(self) -> Tensor:
        """The dense (dSGD-mean) part of the gradient as one contiguous fp32 range: the flat
        range itself, or gathered into ``_dense_buf`` (scatter back with ``_dense_back``)."""
        grad = self.flat.grad
        if self._dense_idx is None:
            a, b = self._dense_ranges[0]
            return grad[a:b]
        torch.index_select(grad, 0, self._dense_idx, out=self._dense_buf)
        return self._dense_buf

    def _dense_back(self, buf: Tensor):
        if self._dense_idx is not None:
            self.flat.grad.index_copy_(0, self._dense_idx, buf)

    def _dense_start(self):
        """Peer exchange: push the dense part right after the backward (no wait), so it crosses
        the links while the power iteration runs; ``_fast_reduce`` finishes it."""
        self._dense_pending = None
        if not (self.peer and self.group.distributed and self._dense_ranges):
            return
        buf = self._dense_view()
        pm = self._peer_mean(("dense",), buf.numel())
        pm.start(buf)
        self._dense_pending = (pm, buf)

    def power_iterations(self) -> Optional[List[int]]:
        """Cumulative power iterations each factorised layer ran on the device (``dad_tol``
        stops a layer early; ``dad_num_pow_iters`` bounds it), or None off the device path."""
        if not (self.fast and getattr(self, "fast_layers", None)):
            return None
        return self._table.iterations()

    def _fast_reduce(self) -> float:
        g = self.group
        W = g.world
        self.comm_bytes = 0
        # (not consumed: a pre_reduce captured in a graph pushes at every replay, and every
        # reduction after it finishes that push)
        pend = getattr(self, "_dense_pending", None)
        if pend is not None:  # pushed before the power iteration (peer)
            pm, buf = pend
            pm.finish(buf)
            self._dense_back(buf)
            self.comm_bytes += pm.bytes_sent
        elif g.distributed and self._dense_ranges:
            buf = self._dense_view()
            self._allreduce_mean_(buf, tag=("dense",))
            self._dense_back(buf)
        if not self.fast_layers:
            return 1.0
        if g.distributed:
            if self.peer:  # one-sided writes into every site's gather slot (fp32 out)
                from . import peer as _peer
                pg = _peer.gather(g, self.flat.grad.device, self._send.numel(), self.wire,
                                  ("rankDAD", "factors"))
                self.comm_bytes += pg.run(self._send, self._gathered, self._send.numel())
            elif self.half:  # factors on the wire in the payload type, reconstructed in fp32
                n = self._send.numel()
                to_payload(self._send, self._send16, 1, n)
                g.all_gather_into(self._gathered16, self._send16)
                from_payload(self._gathered16, self._gathered)
                self.comm_bytes += self._send16.numel() * self._send16.element_size()
            else:
                g.all_gather_into(self._gathered, self._send)
                self.comm_bytes += self._send.numel() * 4
        # every layer's G = [P_1..P_W][Q_1..Q_W]^T / W in one launch
        self._recon.run(self._send.numel(), W if g.distributed else 1)
        return 1.0

    def step_context(self):
        if self.fast:
            return contextlib.nullcontext()
        self._cap = _cap.DADCapture(modules=self.linears)
        return self._cap

    def _dense_pack(self) -> Tensor:
        g = self.flat.grad
        return torch.cat([g[o:o + n] for o, n in self.dense_segs]) if self.dense_segs else g[:0].clone()

    def _dense_unpack(self, buf: Tensor):
        g = self.flat.grad
        off = 0
        for o, n in self.dense_segs:
            g[o:o + n].copy_(buf[off:off + n])
            off += n

    def _layer_inputs(self):
        """Per captured Linear: concatenated ``(A [N, in], Delta [N, out])``."""
        recs = self._cap.records if self._cap is not None else {}
        out = []
        for m in self.linears:
            r = recs.get(m)
            if not r:
                continue
            A = torch.cat([a.reshape(-1, a.shape[-1]) for a, _ in r]).float()
            D = torch.cat([d.reshape(-1, d.shape[-1]) for _, d in r]).float()
            out.append((m, A, D))
        return out

    def _exact(self, A: Tensor, D: Tensor) -> bool:
        # decided from the layer shape only, so every site picks the same mode (the collective
        # layouts must agree); at r >= rank(G) the power iteration is exact anyway
        return self.rank >= min(A.shape[1], D.shape[1])

    def local_factors(self):
        """[(module, mode, X, Y)] with mode 'exact' (X=Delta, Y=A) or 'lowrank' (X=P, Y=Q)."""
        res = []
        k = self.group.replicas
        for m, A, D in self._layer_inputs():
            if self._exact(A, D):
                res.append((m, "exact", D, A))
            else:
                if k > 1:  # the site's gradient: its replicas' rows, G = sum_r D_r^T A_r / k
                    D = self.group.site_all_gather_varlen(D) / k
                    A = self.group.site_all_gather_varlen(A)
                P, Q = dad_factors(D, A, self.rank, self.iters, self.tol)
                res.append((m, "lowrank", P, Q))
        return res

    def reduce(self, factorized: bool = False) -> float:
        """``factorized``: :meth:`pre_reduce` already ran (inside the captured step)."""
        if self.fast:
            if not factorized:
                self.pre_reduce()
            return self._fast_reduce()
        g = self.group
        self.comm_bytes = 0
        dense = self._dense_pack()
        self._allreduce_mean_(dense)
        self._dense_unpack(dense)
        facs = self.local_factors()
        W = g.world
        low = [(m, X, Y) for m, mode, X, Y in facs if mode == "lowrank"]
        if low:
            flat = torch.cat([torch.cat([X.reshape(-1), Y.reshape(-1)]) for _, X, Y in low])
            if self.half:
                flat = flat.to(PAYLOAD_TYPES[self.wire][1])
            gathered = torch.empty(W * flat.numel(), dtype=flat.dtype, device=flat.device)
            g.all_gather_into(gathered, flat)
            self.comm_bytes += flat.numel() * flat.element_size()
            gathered = gathered.view(W, -1).float()
            off = 0
            for m, X, Y in low:
                nx, ny = X.numel(), Y.numel()
                Ps = gathered[:, off:off + nx].reshape(W, *X.shape)
                Qs = gathered[:, off + nx:off + nx + ny].reshape(W, *Y.shape)
                off += nx + ny
                # mean_s P_s Q_s^T  ==  [P_1..P_W] [Q_1..Q_W]^T / W  (one GEMM)
                Pc = Ps.permute(1, 0, 2).reshape(X.shape[0], -1)
                Qc = Qs.permute(1, 0, 2).reshape(Y.shape[0], -1)
                m.weight.grad.copy_((Pc @ Qc.t()).div_(W).view_as(m.weight))
        for m, mode, D, A in facs:
            if mode != "exact":
                continue
            Dc = g.all_gather_varlen(D)
            Ac = g.all_gather_varlen(A)
            self.comm_bytes += (D.numel() + A.numel()) * 4
            m.weight.grad.copy_((Dc.t() @ Ac).div_(W).view_as(m.weight))
        if self._cap is not None:
            self._cap.clear()
        return 1.0

    # file transport
    def payload(self):
        out = {"dense": self._dense_pack()}
        facs = self.local_factors()
        self._captured_order = [m for m, _, _, _ in facs]
        for i, (m, mode, X, Y) in enumerate(facs):
            out[f"L{i:03d}.{mode}.X"] = X
            out[f"L{i:03d}.{mode}.Y"] = Y
        if self._cap is not None:
            self._cap.clear()
        return out

    @classmethod
    def aggregate(cls, payloads, cfg=None):
        W = len(payloads)
        agg = {"dense": sum(p["dense"].float() for p in payloads) / W}
        keys = sorted({k.rsplit(".", 1)[0] for p in payloads for k in p if k != "dense"})
        for k in keys:
            X = torch.cat([p[k + ".X"].float() for p in payloads], 1 if ".lowrank" in k else 0)
            Y = torch.cat([p[k + ".Y"].float() for p in payloads], 1 if ".lowrank" in k else 0)
            agg[k] = (X @ Y.t() / W) if ".lowrank" in k else (X.t() @ Y / W)
        return agg

    def apply(self, agg):
        self._dense_unpack(agg["dense"].to(self.flat.grad.device))
        by_layer = {int(k.split(".")[0][1:]): k for k in agg if k != "dense"}
        for i, k in sorted(by_layer.items()):
            m = self._captured_order[i]
            m.weight.grad.copy_(agg[k].to(m.weight.grad.device).view_as(m.weight))
        return 1.0


# =============================================================================================
# PowerSGD
# =============================================================================================
class PowerSGDEngine(Engine):
    name = "powerSGD"

    def __init__(self, model, flat, group, cfg=None):
        super().__init__(model, flat, group, cfg)
        self.rank = int(self.cfg.get("powersgd_rank", 4))
        self.warm = bool(self.cfg.get("powersgd_warm_start", True))
        self.mats = []   # (param, n, m, r)
        dense = []
        for p, o, n in flat.segments():
            if p.dim() >= 2:
                rows, cols = p.shape[0], p.numel() // p.shape[0]
                r = min(self.rank, rows, cols)
                if (rows + cols) * r < rows * cols:
                    self.mats.append((p, rows, cols, r))
                    continue
            dense.append((o, n))
        self.dense_segs = dense
        gen = torch.Generator(device="cpu").manual_seed(int(self.cfg.get("seed", 0)) + 12345)
        dev = flat.data.device
        # GPU: every matrix of the model per launch (csrc/kernels/lowrank.hip): P = M Q with
        # M = G + err formed in the same pass, Cholesky QR (fp64 Gram) + Q = M^T P, then G = P Q^T and the
        # error feedback -- three launches and two all-reduces per step, no host sync
        self.fast = bool(flat.data.is_cuda and self.warm and _lib.native_available()
                         and self.cfg.get("powersgd_device", True) and self.mats)
        qs = [torch.randn(c, r, generator=gen) for _, _, c, r in self.mats]
        if not self.fast:
            self.Q = [q.to(dev) for q in qs]
            self.err = [torch.zeros(rw, c, device=dev) for _, rw, c, _ in self.mats]
            return
        seg = {id(p): o for p, o, _ in flat.segments()}
        rows_r = sum(rw * r for _, rw, _, r in self.mats)
        self._qbuf = torch.cat([q.reshape(-1) for q in qs]).to(dev)  # Q: warm start + Q all-reduce
        self._pbuf = torch.zeros(rows_r, dtype=torch.float32, device=dev)   # raw P: all-reduce
        self._psend = torch.zeros(rows_r, dtype=torch.float32, device=dev)  # orthonormal P
        self._ebuf = torch.zeros(sum(rw * c for _, rw, c, _ in self.mats), dtype=torch.float32,
                                 device=dev)
        self.Q, self.err, layers = [], [], []
        po = qo = eo = 0
        for p, rw, c, r in self.mats:
            Q = self._qbuf[qo:qo + c * r].view(c, r)
            E = self._ebuf[eo:eo + rw * c].view(rw, c)
            P = self._pbuf[po:po + rw * r].view(rw, r)
            Ps = self._psend[po:po + rw * r].view(rw, r)
            G = flat.grad[seg[id(p)]:seg[id(p)] + rw * c].view(rw, c)
            self.Q.append(Q)
            self.err.append(E)
            layers.append((G, E, P, Ps, Q))
            po, qo, eo = po + rw * r, qo + c * r, eo + rw * c
        self._table = LowRankTable(layers, dev)
        if self.peer:  # the exchanges, built outside any capture (peer.PeerArena)
            nd = sum(n for _, n in self.dense_segs)
            if nd:
                self._peer_mean(("dense",), nd)
            self._peer_mean(("P",), self._pbuf.numel())
            self._peer_mean(("Q",), self._qbuf.numel())

    def pre_reduce(self):
        """M = G + err and the local P = M Q of every matrix (one launch, graph-capturable)."""
        if self.fast:
            self._table.gq(0)

    def state_dict(self):
        return {"Q": [q.detach().cpu().clone() for q in self.Q],
                "err": [e.detach().cpu().clone() for e in self.err]}

    def load_state_dict(self, sd):
        for dst, key in ((self.Q, "Q"), (self.err, "err")):
            for t, v in zip(dst, sd.get(key, [])):
                t.copy_(v.to(t.device))

    def _dense_pack(self):
        g = self.flat.grad
        return torch.cat([g[o:o + n] for o, n in self.dense_segs]) if self.dense_segs else g[:0].clone()

    def _dense_unpack(self, buf):
        g = self.flat.grad
        off = 0
        for o, n in self.dense_segs:
            g[o:o + n].copy_(buf[off:off + n])
            off += n

    def reduce(self, factorized: bool = False) -> float:
        """``factorized``: :meth:`pre_reduce` already ran (inside the captured step)."""
        g = self.group
        W = g.world
        self.comm_bytes = 0
        dense_pm = None
        if g.distributed:
            dense = self._dense_pack()
            if self.peer and self.fast and self.mats and dense.numel():
                # the peer exchange: push the dense part now, finish it after the P / Q rounds
                dense_pm = self._peer_mean(("dense",), dense.numel())
                dense_pm.start(dense)
            else:
                self._allreduce_mean_(dense, tag=("dense",))
                self._dense_unpack(dense)
        if not self.mats:
            return 1.0
        if self.fast:
            if not factorized:
                self.pre_reduce()
            self._allreduce_mean_(self._pbuf, tag=("P",))  # round 1: P (mean over sites)
            self._table.orth_gtp(0)                         # orthonormalise P, Q = M^T P
            self._allreduce_mean_(self._qbuf, tag=("Q",))  # round 2: Q (mean); next warm start
            self._table.recon_ef()                          # G = P Q^T, err = M - G
            if dense_pm is not None:
                dense_pm.finish(dense)
                self._dense_unpack(dense)
                self.comm_bytes += dense_pm.bytes_sent
            return 1.0
        Ms = []
        for (p, rows, cols, r), e in zip(self.mats, self.err):
            M = p.grad.reshape(rows, cols) + e
            Ms.append(M)
        if not self.warm:
            for q in self.Q:
                q.normal_()
        Ps = [M @ q for M, q in zip(Ms, self.Q)]
        pbuf = torch.cat([P.reshape(-1) for P in Ps])
        if g.distributed:
            g.all_reduce(pbuf)
            pbuf.div_(W)
            self.comm_bytes += pbuf.numel() * 4
        off = 0
        for i, P in enumerate(Ps):
            Ps[i] = pbuf[off:off + P.numel()].view_as(P)
            off += P.numel()
        orthonormalize_(Ps)
        Qs = [M.t() @ P for M, P in zip(Ms, Ps)]
        qbuf = torch.cat([Q.reshape(-1) for Q in Qs])
        if g.distributed:
            g.all_reduce(qbuf)
            qbuf.div_(W)
            self.comm_bytes += qbuf.numel() * 4
        off = 0
        for i, (Q, M, P) in enumerate(zip(Qs, Ms, Ps)):
            Qn = qbuf[off:off + Q.numel()].view_as(Q)
            off += Q.numel()
            self.Q[i].copy_(Qn)
            Mh = P @ Qn.t()
            self.err[i].copy_(M - Mh)
            p = self.mats[i][0]
            p.grad.copy_(Mh.view_as(p))
        return 1.0

    # file transport: two rounds (P then Q) are modelled as one call sequence by the compat layer
    def payload_p(self):
        self._Ms = [p.grad.reshape(rw, c) + e for (p, rw, c, _), e in zip(self.mats, self.err)]
        return {"dense": self._dense_pack(), **{f"P{i}": M @ q for i, (M, q) in enumerate(zip(self._Ms, self.Q))}}

    def payload_q(self, agg_p):
        Ps = [agg_p[f"P{i}"].to(self.flat.data.device).clone() for i in range(len(self.mats))]
        orthonormalize_(Ps)
        self._Ps = Ps
        return {f"Q{i}": M.t() @ P for i, (M, P) in enumerate(zip(self._Ms, Ps))}

    def apply_pq(self, agg_p, agg_q):
        self._dense_unpack(agg_p["dense"].to(self.flat.grad.device))
        for i, ((p, rw, c, _), P) in enumerate(zip(self.mats, self._Ps)):
            Qn = agg_q[f"Q{i}"].to(P.device)
            self.Q[i].copy_(Qn)
            Mh = P @ Qn.t()
            self.err[i].copy_(self._Ms[i] - Mh)
            p.grad.copy_(Mh.view_as(p))
        return 1.0

    @classmethod
    def aggregate(cls, payloads, cfg=None):
        W = len(payloads)
        return {k: sum(p[k].float() for p in payloads) / W for k in payloads[0]}


# =============================================================================================
# top-k sparsification
# =============================================================================================
class TopKEngine(Engine):
    """Magnitude top-k sparsification with error feedback (``ops.topk`` holds the contract).

    Every rank is a contributor: replicas of a site each release the top-k of their own
    gradient, and the divisor is the number of ranks.  One site still sparsifies and keeps the
    residual, with no collective.  A non-finite element always wins the selection, leaves the
    residual and reaches the update (``max_grad_norm`` then skips that step).

    The exchange is one all-gather of ``2k`` 32-bit words per rank: inside the captured step
    through the peer exchange (``dsgd_collective='peer'``, indices sent as fp32 values: exact up
    to 2^24 elements), else host-issued through the process group after the replay."""
    name = "topK"
    releases = "top-k (index, value) pairs, not the dense gradient"

    def __init__(self, model, flat, group, cfg=None):
        super().__init__(model, flat, group, cfg)
        if self.half:
            raise ValueError(f"topK: the pairs travel as int32 indices and fp32 values; a "
                             f"{self.wire} payload (precision_bits=16 / payload_dtype) is not "
                             f"implemented")
        self.ratio = topk_ratio_option(self.cfg)
        grad = flat.grad
        n = grad.numel()
        if n >= 2 ** 31:
            raise ValueError(f"topK: int32 indices address fewer than 2^31 elements, got {n}")
        from ..ops import reference as _ref
        self.k = _ref.topk_k(n, self.ratio)
        # the selection runs on the device (csrc/kernels/topk.hip): the step may capture it
        self.fast = bool(flat.data.is_cuda)
        if self.peer and n > FLOAT_INDEX_MAX:
            self.peer = False  # fp32 index words would not be exact
        self.state = TopKState(grad.device, n, self.k, idx_float=self.peer)
        g = group
        if not g.distributed:
            self.transport = "none (one site)"
        elif self.peer:
            self.transport = "peer gather (captured)"
        else:
            self.transport = "all-gather (host-issued)"
        import logging
        logging.getLogger(__name__).info("topK: k = %d of %d elements (ratio %g), exchange: %s",
                                         self.k, n, self.ratio, self.transport)
        if g.distributed:
            self.state.gather_buffer(g.world)
        if self.peer:  # the exchange region, built outside any capture (peer.PeerArena)
            self._peer_gather()

    def _peer_gather(self):
        from . import peer as _peer
        return _peer.gather(self.group, self.flat.grad.device, 2 * self.k, "fp32",
                            (self.name, "pairs"))

    @property
    def capturable(self) -> bool:
        # the process group's all-gather is issued from the host, after the replay
        return not self.group.distributed or self.peer

    def pre_reduce(self):
        """Select and compact this rank's release (local launches, graph-capturable)."""
        self.state.select(self.flat.grad)

    def reduce(self, factorized: bool = False) -> float:
        """``factorized``: :meth:`pre_reduce` already ran (inside the captured step)."""
        if not factorized:
            self.pre_reduce()
        g, st, grad = self.group, self.state, self.flat.grad
        W = g.world if g.distributed else 1
        if not g.distributed:
            st.combine(1, grad, st.send)
        else:
            gathered = st.gather_buffer(W)
            if self.peer:
                self._peer_gather().run(st.send, gathered, 2 * self.k)
            else:
                g.all_gather_into(gathered, st.send)
            st.combine(W, grad, gathered)
        self.comm_bytes = 8 * self.k
        self.last_scale = 1.0 / W
        return self.last_scale

    def state_dict(self):
        return self.state.state_dict()

    def load_state_dict(self, sd):
        self.state.load_state_dict(sd)

    # file transport: one round, the downlink is the sparse union (at most W k pairs)
    def payload(self):
        self.pre_reduce()
        st = self.state
        return {"idx": st.idx.clone(), "val": st.val.clone(),
                "n": torch.tensor(st.n, dtype=torch.int64)}

    @classmethod
    def aggregate(cls, payloads, cfg=None):
        n = int(payloads[0]["n"])
        out = torch.zeros(n, dtype=torch.float32)
        hit = torch.zeros(n, dtype=torch.bool)
        for p in payloads:  # site order: out[i] = ((+0 + v_0) + v_1) + ...
            idx = p["idx"].cpu().to(torch.int64)
            out[idx] = out[idx] + p["val"].cpu().float()
            hit[idx] = True
        idx = hit.nonzero().reshape(-1)
        return {"idx": idx.to(torch.int32), "val": out[idx],
                "n": torch.tensor(n, dtype=torch.int64),
                "sites": torch.tensor(len(payloads), dtype=torch.int64)}

    def apply(self, agg):
        grad = self.flat.grad
        if int(agg["n"]) != grad.numel():
            raise ValueError(f"topK apply(): an aggregate of {grad.numel()} elements is "
                             f"required, got {int(agg['n'])}")
        grad.zero_()
        grad[agg["idx"].to(grad.device, torch.int64)] = agg["val"].to(grad.device, torch.float32)
        self.last_scale = 1.0 / int(agg["sites"])
        return self.last_scale


# =============================================================================================
# coordinate-wise trimmed mean / median
# =============================================================================================
class TrimmedMeanEngine(Engine):
    """Coordinate-wise trimmed mean over the sites (``ops.trimmed`` holds the contract): every
    rank gathers every site's dense fp32 gradient and, per coordinate, drops the ``b`` smallest
    and the ``b`` largest of the ``W`` values and averages the rest.  ``trim_sites`` gives ``b``;
    ``"median"`` (the default) is ``b = (W - 1) // 2``.

    A NaN sorts to an end, so with ``b >= 1`` up to ``b`` non-finite (or arbitrarily wrong) sites
    per coordinate and sign never reach the update; the per-site counters say how often each site
    was dropped.  It bounds each coordinate, nothing more: it is no privacy mechanism (every site
    sees every site's gradient), and ``b = 0`` is a mean summed in value order.

    The exchange is one all-gather of the ``n`` fp32 words per rank: inside the captured step
    through the peer exchange (``dsgd_collective='peer'``), else host-issued through the process
    group after the replay.  One site: the gradient is left as it is."""
    name = "trimmedMean"
    releases = "each site's dense gradient, compared coordinate by coordinate"

    def __init__(self, model, flat, group, cfg=None):
        super().__init__(model, flat, group, cfg)
        if self.half:
            raise ValueError(f"trimmedMean: the gradients travel as fp32; a {self.wire} payload "
                             f"(precision_bits=16 / payload_dtype) is not implemented")
        if group.replicas > 1:
            raise ValueError(f"trimmedMean: {group.replicas} GPUs per site are not supported: a "
                             f"site's replicas are not independent voters, and the site gradient "
                             f"would have to be formed first")
        self.trim = trim_sites_option(self.cfg)
        grad = flat.grad
        n = grad.numel()
        g = group
        W = g.world if g.distributed else 1
        if W > TRIM_MAX_SITES:
            raise ValueError(f"trimmedMean: at most {TRIM_MAX_SITES} sites, got {W}")
        from ..ops import reference as _ref
        # (one site on the file transport: the remote trims, over the payloads it receives)
        self.b = _ref.trimmed_b(W, self.trim) if g.distributed else 0
        if g.distributed and 2 * self.b >= W:
            raise ValueError(f"trimmedMean: trim_sites = {self.b} drops {2 * self.b} of W = {W} "
                             f"sites per coordinate and keeps none (2 * trim_sites < W is "
                             f"required)")
        # the combine runs on the device (csrc/kernels/trimmed.hip): the step may capture it
        self.fast = bool(flat.data.is_cuda)
        self.state = TrimmedState(grad.device, n, W, self.b)
        self._logged = torch.zeros(W, dtype=torch.int64)  # counts already reported (site log)
        if not g.distributed:
            self.transport = "none (one site)"
        elif self.peer:
            self.transport = "peer gather (captured)"
        else:
            self.transport = "all-gather (host-issued)"
        import logging
        logging.getLogger(__name__).info("trimmedMean: W = %d sites, b = %d dropped at each end "
                                         "(%s), exchange: %s", W, self.b, self.trim,
                                         self.transport)
        if g.distributed:
            if self.state.stride != n:  # (FlatParams pads every segment: never with its buffer)
                raise ValueError("trimmedMean: the flat gradient must hold a multiple of 4 "
                                 "elements (the gathered rows are loaded 16 bytes at a time)")
            self.state.gather_buffer()
        if self.peer:  # the exchange region, built outside any capture (peer.PeerArena)
            self._peer_gather()
        self.last_scale = 1.0

    def _peer_gather(self):
        from . import peer as _peer
        return _peer.gather(self.group, self.flat.grad.device, self.flat.grad.numel(), "fp32",
                            (self.name, "grads"))

    @property
    def capturable(self) -> bool:
        # the process group's all-gather is issued from the host, after the replay
        return not self.group.distributed or self.peer

    def reduce(self) -> float:
        g, st, grad = self.group, self.state, self.flat.grad
        if g.distributed:
            rows = st.gather_buffer()  # [W, stride], stride == n
            if self.peer:
                self._peer_gather().run(grad, rows.view(-1), st.stride)
            else:
                g.all_gather_into(rows.view(-1), grad)
            st.combine(rows, grad)
        self.comm_bytes = 4 * grad.numel()
        self.last_scale = 1.0  # the result is a mean already
        return self.last_scale

    def trimmed_share(self) -> List[float]:
        """Each site's share of trimmed coordinates since the last call: counts delta / (n x
        reduces).  Every reduce drops exactly ``2 b n`` entries, so the number of reduces is read
        off the counters themselves (a replayed graph never passes through ``reduce()``)."""
        now = self.state.counts()
        d = now - self._logged
        self._logged = now
        total = int(d.sum())
        if total <= 0:
            return [0.0] * self.state.W
        return [float(v) * 2 * self.b / total for v in d.tolist()]

    def state_dict(self):
        return self.state.state_dict()

    def load_state_dict(self, sd):
        self.state.load_state_dict(sd)
        self._logged = self.state.counts()

    # file transport: one round; the remote trims over the sites' payloads
    def payload(self):
        g = self.flat.grad
        return {"grad": g.detach().clone(), "n": torch.tensor(g.numel(), dtype=torch.int64)}

    @classmethod
    def aggregate(cls, payloads, cfg=None):
        from ..ops import reference as _ref
        W, n = len(payloads), int(payloads[0]["n"])
        b = _ref.trimmed_b(W, trim_sites_option(dict(cfg or {})))
        if 2 * b >= W:
            raise ValueError(f"trimmedMean: trim_sites = {b} drops {2 * b} of W = {W} sites per "
                             f"coordinate and keeps none (2 * trim_sites < W is required)")
        st = TrimmedState("cpu", n, W, b)
        rows = st.gather_buffer()
        for w, p in enumerate(payloads):  # site order
            v = p["grad"].detach().cpu().reshape(-1)
            if v.dtype != torch.float32 or v.numel() != n:
                raise ValueError(f"trimmedMean aggregate(): {n} fp32 elements per site are "
                                 f"required, site {w} sent {v.numel()} {v.dtype}")
            rows[w, :n].copy_(v)
        out = torch.empty(n, dtype=torch.float32)
        st.combine(rows, out)
        return {"grad": out, "n": torch.tensor(n, dtype=torch.int64), "trimmed": st.counts(),
                "b": torch.tensor(b, dtype=torch.int64)}

    def apply(self, agg):
        grad = self.flat.grad
        if int(agg["n"]) != grad.numel():
            raise ValueError(f"trimmedMean apply(): an aggregate of {grad.numel()} elements is "
                             f"required, got {int(agg['n'])}")
        grad.copy_(agg["grad"].to(grad.device, torch.float32))
        self.last_scale = 1.0
        return self.last_scale


# =============================================================================================
# federated averaging with local steps
# =============================================================================================
class FedAvgEngine(Engine):
    """FedAvg / local SGD (``ops.fedavg`` holds the contract of a round): every site takes
    ``fedavg_local_steps`` updates of its own, then the sites average their parameter differences
    from the model they last agreed on (the anchor) and adopt ``anchor + fedavg_server_lr * mean``
    (through ``fedavg_server_momentum`` when it is on).

    A local update is a one-site step: ``local`` -- a :class:`DSGDEngine` on a one-rank group --
    is the engine the step and the device feed get, so the updates run the one-site step forms
    unchanged (the update inside the captured K-step graph).  :meth:`round` runs between two of
    them on the same stream: one delta launch, ONE site mean of the flat gradient buffer (any
    wire, any collective, as every other mean), one adopt launch.  Adam's moments, BatchNorm
    statistics and the step counter stay local to a site.

    The site loop (``runtime.site``) calls :meth:`begin` where every site holds the same
    parameters and :meth:`round` after every ``fedavg_local_steps``-th update of an epoch and
    after its last, so validation and checkpoints see one model."""
    name = "fedAvg"
    releases = "parameter differences, not a gradient"

    def __init__(self, model, flat, group, cfg=None):
        super().__init__(model, flat, group, cfg)
        from ..config import check_fedavg
        opts = dict(self.cfg)
        check_fedavg(opts)
        if float(self.cfg.get("ema_decay") or os.environ.get("DINUNET_EMA_DECAY", "") or 0) > 0:
            raise ValueError("fedAvg: ema_decay is not supported: every site would average the "
                             "weights of its own local updates, so the averages that validation "
                             "and test score would differ between the sites")
        if group.replicas > 1:
            raise ValueError(f"fedAvg: {group.replicas} GPUs per site are not supported: the "
                             f"local updates are one-site steps, and a site's replicas would "
                             f"have to exchange gradients at every one of them")
        self.local_steps = int(opts["fedavg_local_steps"])
        self.weighting = str(opts["fedavg_weighting"])
        self.eta = float(opts["fedavg_server_lr"])
        self.beta = float(opts["fedavg_server_momentum"])
        # this site's weight: 1 ("uniform"), or set_samples() ("samples")
        self.weight: Optional[float] = 1.0 if self.weighting == "uniform" else None
        self.rounds = 0
        self._restored = False
        self.state = FedAvgState(flat, self.beta)
        solo = SiteGroup(device=flat.data.device, outer=group if group.distributed else None)
        self.local = DSGDEngine(model, flat, solo, self.cfg, overlap=False)
        # the local updates run inside the captured step on the device path
        self.fast = bool(flat.data.is_cuda)
        if self.peer:  # the exchange region, built outside any capture (peer.PeerArena)
            self._peer_mean(("round",), flat.grad.numel())

    def set_samples(self, n_train: int):
        """``fedavg_weighting="samples"``: all-gather the sites' train-split sizes and take this
        site's weight ``fp32(W n_s / sum n)``; every site evaluates the same expression."""
        if self.weighting != "samples":
            return
        sizes = self.group.all_gather_object(int(n_train))
        self.weight = site_weights(sizes)[self.group.rank if self.group.distributed else 0]

    # the local updates -------------------------------------------------------------------------
    def step_context(self):
        return self.local.step_context()

    def reduce(self) -> float:
        """A local update exchanges nothing."""
        return self.local.reduce()

    # rounds --------------------------------------------------------------------------------------
    def begin(self):
        """At a point where every site holds identical parameters (the start of a training phase,
        after a resume): the anchor becomes the parameters; the momentum starts at zero unless a
        checkpoint restored it."""
        self.state.begin()
        if self.state.u is not None and not self._restored:
            self.state.u.zero_()
        self._restored = False

    def _weight(self) -> float:
        if self.weight is None:
            raise RuntimeError("fedAvg: fedavg_weighting='samples' needs set_samples() (the "
                               "sites' train-split sizes) before the first round")
        return self.weight

    def round_due(self, update: int, steps: int) -> bool:
        """Does a round follow the ``update``-th (1-based) of an epoch's ``steps`` updates?
        Every ``fedavg_local_steps``-th and the last: ``ceil(steps / K)`` rounds per epoch."""
        return update % self.local_steps == 0 or update == steps

    def round(self):
        """One round on the current stream: delta, the site mean, adopt.  One site is a world of
        one: the mean is the site's own delta."""
        st = self.state
        st.delta(self._weight())
        self._allreduce_mean_(self.flat.grad, tag=("round",))
        st.adopt(self.eta, self.beta)
        self.rounds += 1

    @property
    def drift(self) -> float:
        """This site's ``||p - a||_2`` at the last round (a host read)."""
        return float(self.state.drift)

    def close(self):
        self.local.close()

    def state_dict(self):
        # (an epoch ends with a round: at every checkpoint the anchor equals the parameters)
        return {"rounds": int(self.rounds), **self.state.state_dict()}

    def load_state_dict(self, sd):
        self.rounds = int(sd.get("rounds", 0))
        self.state.load_state_dict(sd)
        self._restored = sd.get("u") is not None and self.state.u is not None

    # file transport: one round; the phase machines' cadence of rounds is not implemented
    # (compat/nodes.py refuses the engine), the pieces carry the collective path's arithmetic
    def payload(self):
        d = self.state.delta(self._weight())
        out = {"delta": d.detach().clone()}
        d.zero_()
        return out

    @classmethod
    def aggregate(cls, payloads, cfg=None):
        acc = None
        for p in payloads:  # site order: (d_0 + d_1) + ...
            v = p["delta"].detach().cpu().reshape(-1)
            if v.dtype != torch.float32 or (acc is not None and v.numel() != acc.numel()):
                raise ValueError("fedAvg aggregate(): fp32 deltas of one length are required")
            acc = v.clone() if acc is None else acc.add_(v)
        W = len(payloads)
        return {"delta": acc if W == 1 else acc.mul_(torch.tensor(1.0 / W, dtype=torch.float32))}

    def apply(self, agg):
        grad = self.flat.grad
        m = agg["delta"]
        if m.numel() != grad.numel():
            raise ValueError(f"fedAvg apply(): an aggregate of {grad.numel()} elements is "
                             f"required, got {m.numel()}")
        grad.copy_(m.to(grad.device, torch.float32).reshape(-1))
        self.state.adopt(self.eta, self.beta)
        self.rounds += 1
        return 1.0


ENGINES = {"dSGD": DSGDEngine, "rankDAD": RankDADEngine, "powerSGD": PowerSGDEngine,
           "topK": TopKEngine, "trimmedMean": TrimmedMeanEngine, "fedAvg": FedAvgEngine}


def make_engine(name: str, model: nn.Module, flat: FlatParams, group: SiteGroup, cfg: dict) -> Engine:
    try:
        cls = ENGINES[name]
    except KeyError:
        raise ValueError(f"unknown agg_engine {name!r}; expected one of {sorted(ENGINES)}")
    if not cls.supports_dp and dp_options(dict(cfg or {}))[0] > 0:
        raise ValueError(f"dp_clip_norm: the private gradient release is implemented for dSGD "
                         f"only, not agg_engine {name!r} (it shares {cls.releases})")
    if not cls.supports_secure_agg and secure_agg_option(dict(cfg or {})):
        raise ValueError(f"secure_agg: the masked gradient sum is implemented for dSGD only, "
                         f"not agg_engine {name!r} (it shares {cls.releases})")
    return cls(model, flat, group, cfg)
