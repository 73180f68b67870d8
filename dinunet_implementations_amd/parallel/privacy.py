"""Privacy accountant of the differentially private gradient release (``ops.dp``).

The guarantee is stated per site under replace-one-subject adjacency.  Every vector a site
releases is clipped to L2 norm ``c``, so replacing one subject moves it by at most ``2 c``, and
the Gaussian noise added has standard deviation ``sigma c``.  One release is therefore rho-zCDP
with ``rho = (2 c)^2 / (2 (sigma c)^2) = 2 / sigma^2`` (Bun and Steinke 2016, Prop. 1.6), ``T``
releases compose to ``rho T`` (Lemma 1.7), and rho-zCDP implies ``(rho + 2 sqrt(rho ln(1 / delta)),
delta)``-DP (Prop. 1.3).  No subsampling amplification is claimed: batches are sequential passes
over the site's data, not random samples.  ``sigma = 0`` gives ``inf``.
"""
from __future__ import annotations

import math
from typing import Optional

ADJACENCY = "replace-one-subject"


def rho_per_release(sigma: float) -> float:
    """zCDP parameter of one release at noise multiplier ``sigma`` (sensitivity ``2 c``)."""
    sigma = float(sigma)
    if not (sigma >= 0.0) or math.isinf(sigma):
        raise ValueError(f"noise multiplier must be a finite number >= 0, got {sigma!r}")
    return math.inf if sigma == 0.0 else 2.0 / (sigma * sigma)


def rho(releases: int, sigma: float) -> float:
    """zCDP parameter of ``releases`` composed releases (adds across phases)."""
    T = int(releases)
    if T < 0:
        raise ValueError(f"releases must be >= 0, got {releases!r}")
    return 0.0 if T == 0 else T * rho_per_release(sigma)


def epsilon_of_rho(rho_total: float, delta: float) -> float:
    """``epsilon`` of ``(epsilon, delta)``-DP implied by ``rho_total``-zCDP."""
    delta = float(delta)
    if not (0.0 < delta < 1.0):
        raise ValueError(f"delta must lie in (0, 1), got {delta!r}")
    r = float(rho_total)
    if r < 0.0 or r != r:
        raise ValueError(f"rho must be >= 0, got {rho_total!r}")
    if math.isinf(r):
        return math.inf
    return r + 2.0 * math.sqrt(r * math.log(1.0 / delta))


def epsilon(releases: int, sigma: float, delta: float) -> float:
    """``epsilon(T, sigma, delta) = rho T + 2 sqrt(rho T ln(1 / delta))`` with ``rho = 2 /
    sigma^2``."""
    return epsilon_of_rho(rho(releases, sigma), delta)


def loggable(eps: float) -> Optional[float]:
    """``eps`` for ``logs.json``: ``inf`` becomes None (JSON null)."""
    return None if math.isinf(eps) else float(eps)


__all__ = ["ADJACENCY", "rho_per_release", "rho", "epsilon_of_rho", "epsilon", "loggable"]
