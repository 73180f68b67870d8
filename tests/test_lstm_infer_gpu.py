"""Forward-only LSTM recurrence (``dn_lstm_fwd_infer``: ``fwd_recur`` with ``SAVE = false``).

When no input needs a gradient, ``ops.bilstm`` takes the entry that stores none of ``c_save``,
``hprev`` and ``pre`` and allocates none of them.  A step's arithmetic is the storing kernel's,
so every output is compared with ``torch.equal`` against ``dn_lstm_fwd`` called directly with the
three buffers, on the same packed operands and the same input projection.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
I = 24  # input features of every case


@pytest.fixture(autouse=True)
def _native():
    from dinunet_implementations_amd.ops import _lib
    if not _lib.native_available():
        pytest.fail("gfx950 kernel library not built")


def _params(Hd, ndir, seed=0, scale=0.2):
    g = torch.Generator().manual_seed(seed)
    return [tuple((torch.randn(*s, generator=g) * scale).to(DEV).requires_grad_()
                  for s in ((4 * Hd, I), (4 * Hd,), (4 * Hd, Hd), (4 * Hd,)))
            for _ in range(ndir)]


def _operands(B, S, Hd, ndir, seed=0):
    """(params, bf16 input, packed operands, bf16 input projection): computed once per case, shared
    by the storing and the forward-only call."""
    from dinunet_implementations_amd.ops.gemm import mm_plain
    from dinunet_implementations_amd.ops.lstm import pack_params
    ps = _params(Hd, ndir, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, S, I, generator=g).to(DEV).to(torch.bfloat16)
    packed = pack_params([t for p in ps for t in p], I, x.device)
    xp = mm_plain(x.reshape(B * S, I), packed[0], trans_b=True, out_dtype=torch.bfloat16)
    return ps, x, packed, xp


def _storing(xp, packed, B, S, Hd, ndir, mode):
    """``dn_lstm_fwd`` in its training form (c_save, hprev and fp32 pre given), called directly."""
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops.lstm import padded_hidden
    _, bias_p, whh_p, _, _ = packed
    HD = padded_hidden(Hd)
    GP = 4 * HD
    BR = int(_lib.lib().dn_lstm_rows_per_wg(B, Hd))
    Bp = (B + BR - 1) // BR * BR
    f32 = dict(dtype=torch.float32, device=DEV)
    c_save = torch.empty(ndir, Bp, S, HD, **f32)
    hprev = torch.empty(ndir, Bp, S, HD, dtype=torch.bfloat16, device=DEV)
    pre = torch.empty(B * S, ndir * GP, **f32)
    hT, cT = torch.empty(B, ndir * Hd, **f32), torch.empty(B, ndir * Hd, **f32)
    hmean = torch.empty(B, ndir * Hd, **f32) if mode == "mean" else None
    hseq = torch.empty(Bp, S, ndir * HD, **f32) if mode != "mean" else None
    bsplit = ndir * GP if bias_p.numel() == 2 * ndir * GP else 0
    _lib.call("dn_lstm_fwd", xp.data_ptr(), bias_p.data_ptr(), whh_p.data_ptr(), B, S, Hd, ndir,
              c_save.data_ptr(), hprev.data_ptr(), _lib.ptr(hseq), _lib.ptr(hmean), 1.0 / S,
              hT.data_ptr(), cT.data_ptr(), pre.data_ptr(), bsplit, 0, _lib.stream())
    if mode == "mean":
        return hmean, hT, cT
    return hseq.view(Bp, S, ndir, HD)[:B, :, :, :Hd].reshape(B, S, ndir * Hd), hT, cT


def _calls(monkeypatch):
    """Names of the native launchers ``ops.lstm`` calls from here on."""
    from dinunet_implementations_amd.ops import _lib
    names, real = [], _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", spy)
    return names


def _check(B, S, Hd, ndir, mode, monkeypatch, packed_of=None):
    from dinunet_implementations_amd.ops.lstm import bilstm
    ps, x, packed, xp = _operands(B, S, Hd, ndir)
    if packed_of is not None:
        packed = packed_of(ps, packed)
    want = _storing(xp, packed, B, S, Hd, ndir, mode)
    names = _calls(monkeypatch)
    with torch.no_grad():
        out, (hT, cT) = bilstm(x, ps, reduce=mode, packed=packed, xp=xp)
    assert "dn_lstm_fwd_infer" in names and "dn_lstm_fwd" not in names
    assert out.shape == want[0].shape
    assert torch.isfinite(out).all() and float(out.abs().sum()) > 0
    assert torch.equal(out, want[0])
    assert torch.equal(hT, want[1]) and torch.equal(cT, want[2])


# (B, S, Hd per direction, directions, output mode)
CASES = [
    (5, 12, 32, 2, "mean"),    # padded units (32 of 64), partial workgroup
    (5, 12, 32, 2, "seq"),
    (1, 1, 64, 1, "mean"),     # single row, single step
    (32, 7, 192, 2, "mean"),   # headline geometry, both reduce modes
    (32, 7, 192, 2, "seq"),
    (6, 4, 100, 2, "seq"),     # 128-unit instantiation
    (3, 5, 200, 2, "mean"),    # streamed W_hh: 256 units
    (3, 5, 200, 2, "seq"),
    (4, 4, 300, 2, "mean"),    # 384 units, two unit groups per wave
    (2, 3, 512, 1, "mean"),
    (2, 3, 512, 1, "seq"),
]


@pytest.mark.parametrize("B,S,Hd,ndir,mode", CASES)
def test_forward_only_is_bitwise_the_storing_forward(B, S, Hd, ndir, mode, monkeypatch):
    _check(B, S, Hd, ndir, mode, monkeypatch)


@pytest.mark.parametrize("mode", ["mean", "seq"])
def test_forward_only_8_row_workgroups_many_rows(mode, monkeypatch):
    """1027 rows at 8 per workgroup: 129 workgroups per direction, the last one 3 rows."""
    from dinunet_implementations_amd.ops import _lib
    monkeypatch.setenv("DN_LSTM_BR", "8")
    assert int(_lib.lib().dn_lstm_rows_per_wg(1027, 64)) == 8
    _check(1027, 2, 64, 2, mode, monkeypatch)


@pytest.mark.parametrize("mode", ["mean", "seq"])
@pytest.mark.parametrize("br", ["4", "8", "16"])
@pytest.mark.parametrize("Hd", [40, 100, 192])
def test_forward_only_every_resident_instantiation(Hd, br, mode, monkeypatch):
    """64 / 128 / 192 padded units x 4 / 8 / 16 rows per workgroup x both output modes (with the
    streamed 256 / 384 / 512 cases above: every instantiation at one unit group per wave).  21 rows:
    a partial last workgroup at every row count.  The compiler is free to contract the cell update
    differently per instantiation, so each one is compared."""
    from dinunet_implementations_amd.ops import _lib
    monkeypatch.setenv("DN_LSTM_BR", br)
    assert int(_lib.lib().dn_lstm_rows_per_wg(21, Hd)) == int(br)
    _check(21, 4, Hd, 2, mode, monkeypatch)


def test_forward_only_three_unit_groups_per_wave(tmp_path):
    """``DINUNET_LSTM_UG=3`` (one wave per SIMD at 192 units, 4 rows) is read once per process, so
    its two instantiations are compared in a child process."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import pytest, test_lstm_infer_gpu as T\n"
            "mp = pytest.MonkeyPatch()\n"
            "for mode in ('mean', 'seq'):\n"
            "    T._check(9, 5, 192, 2, mode, mp)\n"
            "mp.undo(); print('ug3 ok')\n" % (os.path.dirname(here), here))
    env = dict(os.environ, DINUNET_LSTM_UG="3")
    env.pop("DN_LSTM_BR", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "ug3 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("B,S,Hd,ndir,mode", [(32, 7, 192, 2, "mean"), (5, 6, 40, 2, "seq"),
                                              (3, 4, 300, 1, "mean")])
def test_forward_only_with_split_bias_images(B, S, Hd, ndir, mode, monkeypatch):
    """The ``PersistentPack`` form: ``b_ih`` and ``b_hh`` as two images summed in the kernel."""
    from dinunet_implementations_amd.ops.lstm import PersistentPack, pack_params

    def split(ps, packed):
        flat = [t for p in ps for t in p]
        pp = PersistentPack(flat, I, DEV)
        half = pp.bias_p.numel() // 2
        for k, keep in ((0, 1), (1, 3)):  # image k holds b_ih (k = 0) or b_hh (k = 1) alone
            one = [t if i % 4 in (0, 2, keep) else torch.zeros_like(t) for i, t in enumerate(flat)]
            pp.bias_p[k * half:(k + 1) * half].copy_(pack_params(one, I, DEV)[1])
        pp.wih_p.copy_(packed[0])
        pp.whh_p.copy_(packed[2])
        pp.whhT_p.copy_(packed[3])
        assert float(pp.bias_p[:half].abs().sum()) > 0 and float(pp.bias_p[half:].abs().sum()) > 0
        return pp.wih_p, pp.bias_p, pp.whh_p, pp.whhT_p, None

    _check(B, S, Hd, ndir, mode, monkeypatch, packed_of=split)


def test_forward_only_allocates_no_backward_buffers(monkeypatch):
    """B = 64, S = 64, 192 units, 2 directions, on a precomputed projection: the no-grad call's
    peak allocation stays below the bytes of c_save + hprev (``ndir * Bp * S * HD * 6``: it holds
    only hmean, hT and cT); a call whose parameters need gradients exceeds it (it adds pre)."""
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops.lstm import bilstm, padded_hidden
    B, S, Hd, ndir = 64, 64, 192, 2
    ps, x, packed, xp = _operands(B, S, Hd, ndir)
    BR = int(_lib.lib().dn_lstm_rows_per_wg(B, Hd))
    Bp = (B + BR - 1) // BR * BR
    saved = ndir * Bp * S * padded_hidden(Hd) * 6

    def rise(grad):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.set_grad_enabled(grad):
            out, _ = bilstm(x, ps, reduce="mean", packed=packed, xp=xp)
        torch.cuda.synchronize()
        assert out.requires_grad == grad
        return torch.cuda.max_memory_allocated() - base

    names = _calls(monkeypatch)
    r_eval, r_train = rise(False), rise(True)
    assert names == ["dn_lstm_fwd_infer", "dn_lstm_fwd"]
    assert r_eval < saved < r_train, (r_eval, saved, r_train)
    assert r_eval <= 4 * B * ndir * Hd * 4  # the three [B, ndir*Hd] fp32 outputs, rounded up


def test_entry_refuses_bad_arguments():
    """Host-side checks before any launch (status 1 = DN_BAD_SHAPE)."""
    from dinunet_implementations_amd.ops import _lib
    L = _lib.lib()
    p = torch.zeros(64, device=DEV).data_ptr()
    ok = (p, p, p)
    assert L.dn_lstm_fwd_infer(*ok, 4, 3, 600, 2, None, p, 1.0, p, p, 0, None) == 1  # hidden > 512
    assert L.dn_lstm_fwd_infer(*ok, 0, 3, 64, 2, None, p, 1.0, p, p, 0, None) == 1   # empty batch
    assert L.dn_lstm_fwd_infer(*ok, 4, 3, 64, 3, None, p, 1.0, p, p, 0, None) == 1   # directions
    assert L.dn_lstm_fwd_infer(*ok, 4, 3, 64, 2, None, p, 1.0, p, p, 7, None) == 1   # bias split
    assert L.dn_lstm_fwd_infer(*ok, 4, 3, 64, 2, None, None, 1.0, p, p, 0, None) == 1  # no output
    assert L.dn_lstm_fwd_infer(None, p, p, 4, 3, 64, 2, None, p, 1.0, p, p, 0, None) == 1
