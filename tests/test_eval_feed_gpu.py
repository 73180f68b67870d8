"""``runtime.evalfeed.EvalFeed`` against the host evaluation loop it replaces
(``NNTrainer.evaluate`` over an unshuffled ``DeviceLoader``): the same kernels on the same rows,
so every comparison is exact (``torch.equal`` / ``==``)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# the small ICA model of tests/test_runtime_gpu.py::_ica_root: 16 components, T = 120, W = 10
ICA = dict(task_id="ICA-Classification", num_components=16, window_size=10, window_stride=10,
           temporal_size=120, input_size=32, hidden_size=64, batch_size=8)


@pytest.fixture(autouse=True)
def _native():
    from dinunet_implementations_amd.ops import _lib
    if not _lib.native_available():
        pytest.fail("gfx950 kernel library not built")


def _trainer(seed=0, **ov):
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.tasks import get_task
    cfg = build_config(overrides=dict(ICA, **ov))
    T, _, _ = get_task(cfg["task_id"])
    tr = T(cache=cfg, state={}, device=DEV)
    tr.init_nn(seed=seed)
    return tr


def _ica_data(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 12, 16, 10, generator=g).to(DEV)
    Y = torch.randint(0, 2, (n,), generator=g).to(DEV)
    return X, Y


def _host(tr, X, Y, bs):
    """The host loop's result and its per-batch losses and predictions."""
    from dinunet_implementations_amd.data.loader import DeviceLoader
    res = tr.evaluate(DeviceLoader(X, Y, bs))
    losses, preds = [], []
    tr.eval()
    with torch.no_grad():
        for x, y, ix in DeviceLoader(X, Y, bs):
            it = tr.iteration({"inputs": x, "labels": y, "ix": ix})
            losses.append(it["loss"].detach().reshape(1))
            preds.append(it["prediction"].detach())
    tr.train()
    return res, torch.cat(losses).cpu(), torch.cat(preds).cpu()


def _same(feed, tr, X, Y, bs):
    res, losses, preds = _host(tr, X, Y, bs)
    got = feed.run()
    assert got["out"].shape == res["out"].shape and torch.isfinite(got["out"]).all()
    assert torch.equal(got["out"], res["out"])
    assert torch.equal(got["losses"], losses)
    assert torch.equal(got["pred"].cpu(), preds)
    assert got["averages"].count == res["averages"].count == X.shape[0]
    assert got["averages"].average == res["averages"].average
    assert got["metrics"].scores() == res["metrics"].scores()
    return got


@pytest.mark.parametrize("n", [21, 17, 8, 5])  # two full + tail 5; merged tail 9; one full; short
def test_ica_pass_equals_host_loop_and_reads_nothing_stale(n, tmp_path):
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed, eval_partition
    tr = _trainer()
    X, Y = _ica_data(n)
    feed = EvalFeed(tr, X, Y, 8)
    assert (feed.nfull, feed.tail) == eval_partition(n, 8)
    first = _same(feed, tr, X, Y, 8)
    graphs = dict(feed._graphs)
    assert graphs and _same(feed, tr, X, Y, 8)["out"].equal(first["out"])  # a second pass
    ck = str(tmp_path / "ck.pt")
    tr.save_checkpoint(ck)
    # parameters and BatchNorm running statistics changed in place
    with torch.no_grad():
        for p in tr.parameters():
            p.mul_(1.07).add_(0.003)
        for m in tr.nn["net"].modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.add_(0.05)
                m.running_var.mul_(1.3)
    moved = _same(feed, tr, X, Y, 8)
    assert not torch.equal(moved["out"], first["out"])
    # one fused Adam step on a nonzero gradient
    tr.flat.grad.normal_(generator=torch.Generator(device=DEV).manual_seed(5))
    tr.optimizer.step()
    stepped = _same(feed, tr, X, Y, 8)
    assert not torch.equal(stepped["out"], moved["out"])
    # a checkpoint reload (the best-checkpoint reload before the test pass)
    tr.load_checkpoint(ck)
    assert torch.equal(_same(feed, tr, X, Y, 8)["out"], first["out"])
    assert feed._graphs == graphs  # no recapture anywhere above
    assert feed.passes == 5


def test_ica_layernorm_head():
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    tr = _trainer(norm_layer="layer")
    X, Y = _ica_data(21)
    _same(EvalFeed(tr, X, Y, 8), tr, X, Y, 8)


def test_ica_eval_batch_size_16_equals_host_loop_at_16():
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    tr = _trainer()
    X, Y = _ica_data(37)  # two full batches of 16 + tail 5
    _same(EvalFeed(tr, X, Y, 16), tr, X, Y, 16)


def test_ica_many_graph_replays():
    """33 batches of 2 rows: three replays of the 10-batch graph, a 3-batch remainder graph."""
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    tr = _trainer()
    X, Y = _ica_data(66)
    feed = EvalFeed(tr, X, Y, 2)
    assert feed._plan() == [(2, 10)] * 3 + [(2, 3)]
    _same(feed, tr, X, Y, 2)


def test_pass_leaves_training_state_alone():
    """Two training steps with a pass between them: the second step's loss, the parameters after
    it, Adam's step count and the head's dropout counter equal those of a run without the pass."""
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    X, Y = _ica_data(16)
    Xv, Yv = _ica_data(13, seed=9)

    def run(with_pass):
        tr = _trainer(seed=4)
        feed = EvalFeed(tr, Xv, Yv, 8) if with_pass else None
        net, losses = tr.nn["net"], []
        for k in range(2):
            tr.flat.zero_grad()
            out, loss, pred = tr.forward_loss(X[8 * k:8 * k + 8], Y[8 * k:8 * k + 8])
            loss.backward()
            tr.optimizer.step()
            losses.append(loss.detach().clone())
            if k == 0 and feed is not None:
                g0 = tr.flat.grad.clone()
                feed.run()
                assert torch.equal(tr.flat.grad, g0)
                assert all(m.training for m in net.modules())
        return losses, tr.flat.data.clone(), tr.optimizer.step_count, net.head_spec().rng(DEV).clone()

    a, b = run(True), run(False)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1])
    assert torch.equal(a[1], b[1]) and a[2] == b[2] == 2
    assert torch.equal(a[3], b[3])


@pytest.mark.parametrize("n", [37, 33, 9])  # two full + tail 5; merged tail 17; one short batch
def test_fs_pass_equals_host_loop(n):
    """The FS geometry of the ``fs_data_root`` runs (66 features padded to 72 in HBM, hidden
    256-128-64-32, batch-statistics BatchNorm, hard-label scores from ``pred``), batch 16."""
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    from dinunet_implementations_amd.tasks import get_task
    cfg = build_config(overrides={"task_id": "FS-Classification", "batch_size": 16})
    T, _, _ = get_task(cfg["task_id"])
    tr = T(cache=cfg, state={}, device=DEV)
    tr.init_nn(seed=2)
    g = torch.Generator().manual_seed(3)
    X = torch.rand(n, 66, generator=g).to(DEV)
    Y = torch.randint(0, 2, (n,), generator=g).to(DEV)
    feed = EvalFeed(tr, X, Y, 16)
    assert feed.src.width == 66 and feed.ps.xb.shape[1] == 72 and feed.pack is None
    _same(feed, tr, X, Y, 16)
    with torch.no_grad():
        for p in tr.parameters():
            p.mul_(0.9)
    _same(feed, tr, X, Y, 16)


def test_boundary_launcher_refuses_bad_arguments():
    """Host-side checks of ``dn_eval_boundary`` before any launch, and the struct size check."""
    import ctypes
    from dinunet_implementations_amd.ops import DeviceSource, _lib
    from dinunet_implementations_amd.ops.evalpass import EvalPass, _boundary_type
    Eb = _boundary_type()
    assert ctypes.sizeof(Eb) == _lib.lib().dn_eval_boundary_size()
    src = DeviceSource(torch.zeros(6, 16, dtype=torch.bfloat16, device=DEV),
                       torch.zeros(6, dtype=torch.long, device=DEV), 1)
    ps = EvalPass(src, 4, 2, 2)
    L = _lib.lib()
    assert L.dn_eval_boundary(None, None) == 1

    def rc(**ch):
        kw = dict(out=None, pred=None, loss=None, out_all=ps.out_all.data_ptr(),
                  pred_all=ps.pred_all.data_ptr(), loss_b=ps.loss_b.data_ptr(),
                  cursor=ps.cursor.data_ptr(), ticket=ps.ticket.data_ptr(), gx=src.X.data_ptr(),
                  gy=src.Y.data_ptr(), xb=ps.xb.data_ptr(), yd=ps.yd.data_ptr(), N=6, nb=2, ld=2,
                  C=2, n_prev=0, cap=4, f8=2, mode=1)
        kw.update(ch)
        e = Eb(**kw)
        return L.dn_eval_boundary(ctypes.addressof(e), None)

    assert rc(out_all=None) == 1 and rc(gx=None) == 1 and rc(ticket=None) == 1
    assert rc(n_prev=5) == 1 and rc(n_prev=-1) == 1 and rc(cap=0) == 1 and rc(mode=0) == 1
    assert rc(n_prev=2) == 1                      # a finished batch without its outputs
    assert rc(gx=src.X.data_ptr() + 2) == 1       # misaligned for 16-byte loads
    assert rc(N=0) == 1 and rc(f8=0) == 1
    with pytest.raises(ValueError):
        ps.boundary(torch.zeros(2, 3, device=DEV), torch.zeros((), device=DEV),
                    torch.zeros(2, dtype=torch.long, device=DEV), 2)  # C mismatch
