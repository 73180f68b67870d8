"""A numpy ``float32`` mirror of one federated-averaging round, written from the contract (README
"fedAvg", ``ops/fedavg.py`` docstring), not from the kernels or the torch path it judges.

Per element, every fp32 operation rounded on its own (numpy never fuses a multiply and an add):

* ``delta``: ``d = (p - a) * w``; ``drift = sqrt(sum (p - a)^2)`` in fp64 (unweighted);
* the site mean ``m`` (``mean_site_order``: the fp32 sum in site order times ``fp32(1) / fp32(W)``,
  what the peer exchange, the direct exchange and the file transport form on an fp32 wire;
  ``wire_ref.site_mean`` for any wire; ``mean64`` is the fp64 oracle);
* ``adopt``: with momentum ``u = beta * u + m; s = u``, else ``s = m``; ``a = a + eta * s``;
  ``p = a``; the gradient buffer is zero.

``site_weights``: ``w_s = fp32(W * n_s / sum n)`` evaluated in double.
"""
import numpy as np

f32 = np.float32


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=f32)).view(np.uint32)


def same_bits(got, want):
    """Bit equality; a NaN matches any NaN (host and device give a made NaN other payloads)."""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def delta(p, a, w=1.0):
    """``(d, drift)``."""
    p, a = np.asarray(p, dtype=f32), np.asarray(a, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p - a
        d = t * f32(w)
        t64 = t.astype(np.float64)
        drift = float(np.sqrt(np.sum(t64 * t64)))
    assert t.dtype == f32 and d.dtype == f32
    return d, drift


def adopt(m, a, u=None, eta=1.0, beta=0.0):
    """``(a', p', u', g')``; ``u`` None: no momentum (``beta`` is not read)."""
    m, a = np.asarray(m, dtype=f32), np.asarray(a, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        if u is not None:
            u = f32(beta) * np.asarray(u, dtype=f32) + m
            s = u
        else:
            s = m
        a2 = a + f32(eta) * s
    assert a2.dtype == f32
    return a2, a2.copy(), u, np.zeros_like(a2)


def mean_site_order(ds):
    """The fp32 sum in site order (starting from the first site's value) times ``1 / W``."""
    W = len(ds)
    acc = np.asarray(ds[0], dtype=f32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for d in ds[1:]:
            acc = acc + np.asarray(d, dtype=f32)
        return acc if W == 1 else acc * (f32(1.0) / f32(W))


def mean64(ds):
    return sum(np.asarray(d, dtype=np.float64) for d in ds) / len(ds)


def site_weights(sizes):
    W, tot = len(sizes), sum(int(n) for n in sizes)
    return [f32(W * int(n) / tot) for n in sizes]


def round_(ps, a, us=None, ws=None, eta=1.0, beta=0.0, mean=mean_site_order):
    """One round of ``W`` sites that share the anchor ``a``: returns ``(a', [u'_s], m, [drift_s])``.
    Every site adopts the same mean, so ``a'`` (= every ``p'``) is one vector; the momenta are
    per site (equal when they started equal)."""
    W = len(ps)
    ws = [1.0] * W if ws is None else ws
    dd = [delta(p, a, w) for p, w in zip(ps, ws)]
    m = np.asarray(mean([d for d, _ in dd]), dtype=f32)
    outs = [adopt(m, a, None if us is None else us[s], eta, beta) for s in range(W)]
    return outs[0][0], [o[2] for o in outs], m, [dr for _, dr in dd]
