"""Key agreement of the secure aggregation (``ops.secagg``): every pair of parties derives one
256-bit mask key per (fold, phase) from an ephemeral X25519 exchange.  Host only, standard
library only.

* X25519 (RFC 7748) over Python ints: the Montgomery ladder on Curve25519, scalars clamped as the
  RFC prescribes.  Python's big-integer arithmetic is not constant time; the exchange runs once
  per (fold, phase) on the party's own host, where timing is not observable by the peers.
* an ephemeral key pair per (fold, phase) from ``secrets``; ONE ``all_gather`` of the 32-byte
  public keys over the process group;
* ``k_ij = SHA-256(b"dinunet-secagg-v1" || min(pk_i, pk_j) || max(pk_i, pk_j) || shared || fold
  || phase)`` (fold and phase as 4-byte little-endian words).

The exchange is unauthenticated (parties are honest but curious: nobody substitutes a key in
transit), and there is no dropout recovery.  Keys are returned to the caller, who writes them into
the device block (``SecAggState``) and keeps no other copy; nothing here logs or stores them.
"""
from __future__ import annotations

import hashlib
import secrets
import struct
from typing import List, Optional, Sequence, Tuple

P = 2 ** 255 - 19
A24 = 121665
BASE = (9).to_bytes(32, "little")
LABEL = b"dinunet-secagg-v1"


def _clamp(k: bytes) -> int:
    if len(k) != 32:
        raise ValueError("x25519: a 32-byte scalar is required")
    e = bytearray(k)
    e[0] &= 248
    e[31] &= 127
    e[31] |= 64
    return int.from_bytes(e, "little")


def x25519(k: bytes, u: bytes) -> bytes:
    """RFC 7748 ``X25519(k, u)``: scalar ``k`` and u-coordinate ``u``, 32 bytes each."""
    if len(u) != 32:
        raise ValueError("x25519: a 32-byte u-coordinate is required")
    kk = _clamp(k)
    x1 = int.from_bytes(u, "little") & ((1 << 255) - 1)
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (kk >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) % P
        x3 = x3 * x3 % P
        z3 = (da - cb) % P
        z3 = x1 * (z3 * z3 % P) % P
        x2 = aa * bb % P
        z2 = e * ((aa + A24 * e) % P) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def keypair(private: Optional[bytes] = None) -> Tuple[bytes, bytes]:
    """``(private, public)``: a fresh ephemeral pair from ``secrets`` (or the pair of a given
    32-byte private scalar)."""
    sk = secrets.token_bytes(32) if private is None else bytes(private)
    return sk, x25519(sk, BASE)


def pair_key(sk: bytes, pk_mine: bytes, pk_peer: bytes, fold: int, phase: int) -> bytes:
    """``k_ij`` as this end derives it (both ends get the same 32 bytes)."""
    shared = x25519(sk, pk_peer)
    if shared == bytes(32):  # a low-order public key: the secret would be known to everybody
        raise ValueError("secure_agg: a peer sent a public key of low order")
    lo, hi = (pk_mine, pk_peer) if pk_mine <= pk_peer else (pk_peer, pk_mine)
    return hashlib.sha256(LABEL + lo + hi + shared
                          + struct.pack("<II", int(fold) & 0xFFFFFFFF, int(phase) & 0xFFFFFFFF)
                          ).digest()


def derive_keys(sk: bytes, publics: Sequence[bytes], rank: int, fold: int,
                phase: int) -> List[Optional[bytes]]:
    """This party's key table from everybody's public keys: entry ``j`` is ``k_{rank, j}``
    (``None`` at ``rank``)."""
    pk = publics[rank]
    if len(set(bytes(p) for p in publics)) != len(publics):
        raise ValueError("secure_agg: two parties sent the same public key")
    return [None if j == rank else pair_key(sk, pk, bytes(p), fold, phase)
            for j, p in enumerate(publics)]


def agree(group, fold: int = 0, phase: int = 0) -> List[Optional[bytes]]:
    """One key agreement over ``group``: an ephemeral pair, one ``all_gather`` of the public
    keys, the pair keys of this rank.  Every rank of the group is a party."""
    sk, pk = keypair()
    publics = [bytes(p) for p in group.all_gather_object(pk)]
    if any(len(p) != 32 for p in publics) or publics[group.rank] != pk:
        raise ValueError("secure_agg: malformed public keys from the process group")
    return derive_keys(sk, publics, group.rank, fold, phase)
