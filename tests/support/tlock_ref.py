"""Reference values of the timelock opening, from the Python oracle alone: TEST INFRASTRUCTURE ONLY.

The engine returns E = e(U, sigma)^3 (include/blsverify.h "timelock") as twelve canonical Fp values,
48 bytes big-endian each, highest tower coefficient first. One oracle pairing costs about a second in
pure Python, so the tests take ONE pairing per signature, G = e(G1, sigma)^3, and derive every other
expected value as G^r for U = r * G1 (bilinearity).

Also the encryptor the engine does not have (clients encrypt one message at a time):
U = r * G1, K = (e(pk, H(MessageV2(round)))^3)^r, C = m XOR kdf(encode(K)).
"""
from __future__ import annotations

import functools
import hashlib

from oracle import bls12381 as O

GT_LEN = 576
GT_ONE = bytes(GT_LEN - 1) + b"\x01"


def encode_gt(a):
    """The 576 bytes of an oracle Fp12 value (polynomial form [c0..c5] in w, Fp2 coefficients)."""
    (a0, a1, a2), (b0, b1, b2) = O.to_tower(a)  # c0 = (a0, a1, a2), c1 = (b0, b1, b2)
    out = b""
    for re, im in (b2, b1, b0, a2, a1, a0):
        out += (im % O.P).to_bytes(48, "big") + (re % O.P).to_bytes(48, "big")
    return out


def gt_base(sig_pt):
    """G = e(G1, sigma)^3 for the decoded signature point (None = infinity -> 1)."""
    return O.f12_pow(O.pairing(O.G1, sig_pt), 3)


def gt_pow(base, r):
    return O.f12_pow(base, r % O.R)


def u_of(r):
    """compress(r * G1); r = 0 is the point at infinity."""
    return O.g1_compress(O.g1_mul(O.G1, r % O.R) if r % O.R else None)


def consecutive_us(n):
    """compress((i + 1) * G1) for i < n: Jacobian mixed additions of G1 and ONE inversion for all
    (Montgomery's trick) -- the oracle's affine addition inverts per point."""
    p = O.P
    x2, y2 = O.G1
    two = O.g1_add(O.G1, O.G1)
    jac = [(x2, y2, 1), (two[0], two[1], 1)][:n]
    while len(jac) < n:
        x1, y1, z1 = jac[-1]
        zz = z1 * z1 % p
        h = (x2 * zz - x1) % p
        r = (y2 * z1 * zz - y1) % p
        hh = h * h % p
        hhh = h * hh % p
        v = x1 * hh % p
        x3 = (r * r - hhh - 2 * v) % p
        jac.append((x3, (r * (v - x3) - y1 * hhh) % p, z1 * h % p))
    pre, acc = [], 1
    for _, _, z in jac:
        pre.append(acc)
        acc = acc * z % p
    inv = O.fp_inv(acc)
    out = [None] * n
    for k in range(n - 1, -1, -1):
        x, y, z = jac[k]
        zi = inv * pre[k] % p
        inv = inv * z % p
        zi2 = zi * zi % p
        out[k] = O.g1_compress((x * zi2 % p, y * zi2 * zi % p))
    assert out[-1] == u_of(n)
    return out


def running_gts(base, n):
    """encode(base^(i + 1)) for i < n by a running product."""
    out, acc = [], O.F12_ONE
    for _ in range(n):
        acc = O.f12_mul(acc, base)
        out.append(encode_gt(acc))
    return out


def encrypt(pk_pt, round_, msg, r, kdf):
    """(U48, C) of `msg` locked to `round_` under the group key point pk_pt with the ephemeral scalar r.
    e(r G1, s H) = e(pk, H)^r, so whoever holds sigma = s H(MessageV2(round)) opens it."""
    h = O.hash_to_g2(O.message_v2(round_))
    k = gt_pow(O.f12_pow(O.pairing(pk_pt, h), 3), r)
    ks = kdf(encode_gt(k), len(msg))
    return u_of(r), bytes(a ^ b for a, b in zip(msg, ks))


def g1_class(buf):
    """oracle.g1_decompress's verdict as a BLSV_REJ_* class (0 = decodes)."""
    try:
        O.g1_decompress(buf)
        return 0
    except O.DecodeError as e:
        return e.cls


@functools.lru_cache(maxsize=None)
def bad_us():
    """One compressed G1 encoding per decode reject class 2..6: {class: 48 bytes} (do not modify)."""
    gen = O.g1_compress(O.G1)
    out = {
        O.REJ_FLAG: bytes([gen[0] & 0x7F]) + gen[1:],
        O.REJ_INF_NONZERO: b"\xc0" + bytes(46) + b"\x01",
        O.REJ_X_GE_P: bytes([0x80 | (O.P >> 376)]) + (O.P % (1 << 376)).to_bytes(47, "big"),
    }
    x = 1
    while O.REJ_NOT_ON_CURVE not in out or O.REJ_NOT_IN_SUBGROUP not in out:
        x += 1
        y = O.fp_sqrt((x * x * x + O.B1) % O.P)
        enc = bytearray(x.to_bytes(48, "big"))
        enc[0] |= 0x80
        if y is None:
            out.setdefault(O.REJ_NOT_ON_CURVE, bytes(enc))
        elif not O.g1_in_subgroup((x, y)):  # a curve point found by trial x: almost never in the subgroup
            out.setdefault(O.REJ_NOT_IN_SUBGROUP, bytes(enc))
    for c, b in out.items():
        assert g1_class(b) == c, (c, b.hex())
    return out


def bad_sigs(good_sig):
    """One compressed G2 encoding per decode reject class 2..6, derived from a valid signature."""
    from oracle import c_oracle as C
    out = {
        O.REJ_FLAG: bytes([good_sig[0] & 0x7F]) + good_sig[1:],
        O.REJ_INF_NONZERO: b"\xc0" + bytes(94) + b"\x01",
        O.REJ_X_GE_P: bytes([0x80 | (O.P >> 376)]) + (O.P % (1 << 376)).to_bytes(47, "big") + bytes(48),
    }
    x0 = 1
    while O.REJ_NOT_ON_CURVE not in out or O.REJ_NOT_IN_SUBGROUP not in out:
        x0 += 1
        enc = bytearray(bytes(48) + x0.to_bytes(48, "big"))  # x = (x0, 0): c1 first on the wire
        enc[0] |= 0x80
        c = C.g2_decode_class(bytes(enc))
        if c in (O.REJ_NOT_ON_CURVE, O.REJ_NOT_IN_SUBGROUP):
            out.setdefault(c, bytes(enc))
    for c, b in out.items():
        assert C.g2_decode_class(b) == c, (c, b.hex())
    return out


class OracleTlockEngine:
    """Stand-in for the two Engine methods callers.timelock_open uses, answered by the oracle: one
    pairing per distinct signature, every U = r * G1 looked up by its known r (`scalars`: {U48: r})."""

    def __init__(self, pk48, scalars):
        from oracle import c_oracle
        self.c = c_oracle
        self.pk = bytes(pk48)
        self.scalars = dict(scalars)
        self.bases = {}
        self.calls = []

    def verify_unchained(self, sigs, first_round=None, rounds=None):
        from drand_amd.engine import BatchResult
        self.calls.append("verify_unchained")
        cls = [self.c.verify(self.pk, O.message_v2(first_round + i), bytes(s)) for i, s in enumerate(sigs)]
        bad = [i for i, c in enumerate(cls) if c]
        return BatchResult([c == 0 for c in cls], bad[0] if bad else None, cls)

    def tlock_open(self, sig, us):
        from drand_amd.engine import TlockResult
        self.calls.append("tlock_open")
        sig = bytes(sig)
        if sig not in self.bases:
            self.bases[sig] = gt_base(O.g2_decompress(sig))
        cls = [g1_class(u) for u in us]
        gt = [encode_gt(gt_pow(self.bases[sig], self.scalars[bytes(u)])) if c == 0 else None for u, c in zip(us, cls)]
        return TlockResult([c == 0 for c in cls], cls, gt)


def sha_kdf(gt, n):
    """A second KDF for the tests that must show the callers pass `kdf` through."""
    return hashlib.shake_128(gt).digest(n)
