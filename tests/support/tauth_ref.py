"""Reference values of the authenticated timelock (include/blsverify.h "authenticated timelock"), from hashlib
and Python integers alone: TEST INFRASTRUCTURE ONLY.

A ciphertext of M under the seed s is (U, V, W): k = H3(s, M), U = compress(k G1), K = base^k,
V = s XOR H2(encode(K)), W = M XOR H4(s, len(M)). U and K come from tlock_ref (u_of, gt_pow, encode_gt) over the
ONE oracle pairing a module takes for its base.
"""
from __future__ import annotations

import hashlib

from oracle import bls12381 as O
from tests.support import tlock_ref as T

TAG3 = b"BLSV-TLOCK-FO-H3"
TAG4 = b"BLSV-TLOCK-FO-H4"
SEED_LEN = 32
V_LEN = 32
REJ_TLOCK_AUTH = 10
# the lengths at which the hashing can go wrong (the hashed length is 52 + mlen); DWORD_LENS take the dword stores
MLENS = [1, 3, 4, 11, 12, 13, 32, 33, 67, 68, 76, 255, 256]
DWORD_LENS = [4, 12, 32, 68, 76, 256]


def be32(j):
    return j.to_bytes(4, "big")


def xor(a, b):
    assert len(a) == len(b)
    return bytes(x ^ y for x, y in zip(a, b))


def h3_int(seed, msg):
    """The 384-bit integer H3 reduces."""
    d0 = hashlib.sha256(TAG3 + seed + msg + be32(0)).digest()
    d1 = hashlib.sha256(TAG3 + seed + msg + be32(1)).digest()
    return int.from_bytes(d0 + d1[:16], "big")


def h3(seed, msg):
    assert len(seed) == SEED_LEN
    return h3_int(seed, msg) % O.R


def h2(gt576):
    assert len(gt576) == T.GT_LEN
    return hashlib.sha256(gt576 + be32(0)).digest()


def h4(seed, mlen):
    out, j = b"", 0
    while len(out) < mlen:
        out += hashlib.sha256(TAG4 + seed + be32(j)).digest()
        j += 1
    return out[:mlen]


def seal_tail(seed, msg, gt576):
    """(V, W) of msg under seed given the encoded K."""
    return xor(seed, h2(gt576)), xor(msg, h4(seed, len(msg)))


def encrypt(base, seed, msg):
    """(U, V, W) under the module's base = e(pk, H(MessageV2(round)))^3."""
    k = h3(seed, msg)
    assert k != 0
    v, w = seal_tail(seed, msg, T.encode_gt(T.gt_pow(base, k)))
    return T.u_of(k), v, w


def open_tail(gt576, u48, v, w):
    """The opening's verdict given the encoded E: the message, or None where the check fails. u48 must decode."""
    seed = xor(v, h2(gt576))
    msg = xor(w, h4(seed, len(w)))
    k = h3(seed, msg)
    if k == 0 or T.u_of(k) != bytes(u48) or bytes(u48) == T.u_of(0):
        return None
    return msg


def seed_of(i):
    """The deterministic seed of item i."""
    return hashlib.sha256(b"tauth-test-seed" + i.to_bytes(4, "big")).digest()


def message(i, mlen):
    return bytes((41 * i + 13 * j + 7) % 256 for j in range(mlen))


# ------------------------------------------------------------------ many items: fixed-base forms
# T.u_of / T.gt_pow cost a tenth of a second per item in pure Python; a module that needs 65 items at every
# length takes the same values from four-bit window tables (integers and oracle.f12_mul alone, checked against
# T.u_of / T.gt_pow where they are built).
class FixedBase:
    """base^k for many k: base^(d 16^w), w < 64, d < 16."""

    def __init__(self, base):
        self.rows = []
        b = base
        for _ in range(64):
            row = [O.F12_ONE, b]
            for _d in range(2, 16):
                row.append(O.f12_mul(row[-1], b))
            self.rows.append(row)
            b = O.f12_mul(row[15], b)
        k = O.R - 0x1234567
        assert self.pow(k) == T.gt_pow(base, k)

    def pow(self, k):
        acc, k = None, k % O.R
        for w in range(64):
            d = (k >> (4 * w)) & 15
            if d:
                acc = self.rows[w][d] if acc is None else O.f12_mul(acc, self.rows[w][d])
        return O.F12_ONE if acc is None else acc


def _jac_dbl(pt):
    p = O.P
    x, y, z = pt
    a, b = x * x % p, y * y % p
    c = b * b % p
    d = 2 * ((x + b) * (x + b) - a - c) % p
    e = 3 * a % p
    x3 = (e * e - 2 * d) % p
    return x3, (e * (d - x3) - 8 * c) % p, 2 * y * z % p


def _jac_add_aff(pt, q):
    p = O.P
    x1, y1, z1 = pt
    zz = z1 * z1 % p
    h = (q[0] * zz - x1) % p
    r = (q[1] * z1 * zz - y1) % p
    assert h, "an exceptional addition: not met for k < r in a double-and-add from the top bit"
    hh = h * h % p
    hhh = h * hh % p
    v = x1 * hh % p
    x3 = (r * r - hhh - 2 * v) % p
    return x3, (r * (v - x3) - y1 * hhh) % p, z1 * h % p


def u_of(k):
    """compress(k G1) by a Jacobian double-and-add and one inversion; k != 0 mod r."""
    k %= O.R
    assert k
    acc = None
    for b in range(k.bit_length() - 1, -1, -1):
        if acc is not None:
            acc = _jac_dbl(acc)
        if (k >> b) & 1:
            acc = (O.G1[0], O.G1[1], 1) if acc is None else _jac_add_aff(acc, O.G1)
    x, y, z = acc
    zi = pow(z, -1, O.P)
    zi2 = zi * zi % O.P
    return O.g1_compress((x * zi2 % O.P, y * zi2 * zi % O.P))


def batch(fb, n, mlen):
    """The n-item reference batch at one length: a list of (seed, msg, k, U, V, W), deterministic per item."""
    out = []
    for i in range(n):
        seed, msg = seed_of(i), message(i, mlen)
        k = h3(seed, msg)
        v, w = seal_tail(seed, msg, T.encode_gt(fb.pow(k)))
        out.append((seed, msg, k, u_of(k), v, w))
    assert out[0][3] == T.u_of(out[0][2])
    return out
