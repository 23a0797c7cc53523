"""Shared inputs and expectations of the timelock sealing tests, from the Python oracle and
tests/support/tlock_ref.py alone: TEST INFRASTRUCTURE ONLY.

A seal of scalar k to (pk, round) is U = (k mod r) * G1 and K = B^(k mod r) with
B = e(pk, H(MessageV2(round)))^3; k == 0 (mod r) is refused (zero bytes). One oracle pairing per
(pk, round); every other expectation is a power of it.
"""
from __future__ import annotations

from oracle import bls12381 as O
from tests.support import tlock_ref as T

R = O.R
U_LEN, GT_LEN = 48, 576

FULL = 0xC3A5F00DDEADBEEF0123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A6979  # full width, odd, > r
assert FULL & 1 and FULL >> 255 and FULL % R

# the edge scalars of both suites: window boundaries, the top digit alone, every digit 15 (two
# reductions), r - 1, two values == 1, one full-width odd value, then the three refused values
EDGE = [1, 2, 15, 16, 17, 16 ** 63, 2 ** 256 - 1, R - 1, R + 1, 2 * R + 1, FULL, 0, R, 2 * R]
REFUSED = (0, R, 2 * R)
assert all(0 <= k < 2 ** 256 for k in EDGE)


def be32(k):
    return int(k).to_bytes(32, "big")


def kbase(pk_pt, round_):
    """B = e(pk, H(MessageV2(round)))^3: the one pairing of a (key, round)."""
    return O.f12_pow(O.pairing(pk_pt, O.hash_to_g2(O.message_v2(round_))), 3)


def expect(base, k):
    """(ok, U48, K576) of scalar k under the base; zero bytes for a refused scalar."""
    if k % R == 0:
        return False, bytes(U_LEN), bytes(GT_LEN)
    return True, T.u_of(k % R), T.encode_gt(T.gt_pow(base, k % R))


class Expectations:
    """expect() with the values of repeated scalars (mod r) computed once."""

    def __init__(self, base):
        self.base = base
        self.memo = {}

    def __call__(self, k):
        r = k % R
        if r not in self.memo:
            self.memo[r] = expect(self.base, r)
        return self.memo[r]


def batch65():
    """The 65-item batch of the GPU suite: the edge scalars first, then i + 2, the full-width value
    also in positions 62-64 (both sides of the 64-lane wave boundary)."""
    ks = list(EDGE) + [i + 2 for i in range(len(EDGE), 65)]
    for i in (62, 63, 64):
        ks[i] = FULL
    assert len(ks) == 65
    return ks


class OracleSealEngine(T.OracleTlockEngine):
    """Stand-in for Engine.tlock_seal (beside the opening's stand-in), answered by the oracle: one
    pairing per round; every sealed U is remembered with its scalar so that tlock_open can open it."""

    def __init__(self, pk48):
        super().__init__(pk48, {})
        self.kbases = {}

    def tlock_seal(self, round_, scalars, pk48=None):
        from drand_amd.engine import TsealResult
        self.calls.append("tlock_seal")
        pk = self.pk if pk48 is None else bytes(pk48)
        key = (pk, round_)
        if key not in self.kbases:
            self.kbases[key] = kbase(O.g1_decompress(pk), round_)
        oks, us, gts = [], [], []
        for k in scalars:
            k = int.from_bytes(k, "big") if isinstance(k, (bytes, bytearray)) else int(k)
            ok, u, gt = expect(self.kbases[key], k)
            oks.append(ok)
            us.append(u if ok else None)
            gts.append(gt if ok else None)
            if ok:
                self.scalars[u] = k % R
        return TsealResult(oks, us, gts)
