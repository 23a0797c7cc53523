"""Shared helpers of the tests of the timelock opening across many rounds, from the Python oracle and
tests/support/tlock_ref.py alone: TEST INFRASTRUCTURE ONLY.

Item i of round j opens to e(U_i, sigma_j)^3. One oracle pairing per DISTINCT signature, G_j =
e(G1, sigma_j)^3 (about 0.65 s each in pure Python: a test keeps to at most 4 of them); every other
expectation is G_j^k for U = k * G1.
"""
from __future__ import annotations

from oracle import bls12381 as O
from tests.support import tlock_ref as T

REJ_TLOCK_SIG = 9
MIXED = -1


def plan(counts, cap, dense_min):
    """hostlogic.h open_rounds_next_pass restated: the passes [base, cnt, sig_j, tiles] of `counts` with at
    most `cap` items each; a tile is [first, len, sig], sig an index into the pass's sig_j or MIXED."""
    passes, j, used, base = [], 0, 0, 0
    while True:
        cnt, sig_j, tiles, mixed_from = 0, [], [], 0

        def cut(lo, hi, sig):
            for f in range(lo, hi, 64):
                tiles.append([f, min(64, hi - f), sig])

        while j < len(counts) and cnt < cap:
            left = counts[j] - used
            if left == 0:
                j, used = j + 1, 0
                continue
            take = min(left, cap - cnt)
            sig_j.append(j)
            if take >= dense_min:
                cut(mixed_from, cnt, MIXED)
                cut(cnt, cnt + take, len(sig_j) - 1)
                mixed_from = cnt + take
            cnt += take
            used += take
            if used == counts[j]:
                j, used = j + 1, 0
        cut(mixed_from, cnt, MIXED)
        if cnt == 0:
            return passes
        passes.append([base, cnt, sig_j, tiles])
        base += cnt


class Bases:
    """G = e(G1, sigma)^3 per signature bytes, one pairing each, shared by whoever holds the object."""

    def __init__(self):
        self.memo = {}

    def __call__(self, sig):
        sig = bytes(sig)
        if sig not in self.memo:
            self.memo[sig] = T.gt_base(O.g2_decompress(sig, check_subgroup=False))
        return self.memo[sig]


def expected(bases, sig, ks):
    """The encodings of e(k G1, sigma)^3 for the scalars ks."""
    return [T.encode_gt(T.gt_pow(bases(sig), k)) for k in ks]


class OracleOpenRoundsEngine(T.OracleTlockEngine):
    """OracleTlockEngine with Engine.tlock_open_rounds beside tlock_open, and verify_unchained taking
    `rounds`: answered by the oracle, one pairing per distinct signature."""

    def verify_unchained(self, sigs, first_round=None, rounds=None):
        from drand_amd.engine import BatchResult
        self.calls.append("verify_unchained")
        sigs = list(sigs)
        rounds = [first_round + i for i in range(len(sigs))] if rounds is None else list(rounds)
        cls = [self.c.verify(self.pk, O.message_v2(r), bytes(s)) for r, s in zip(rounds, sigs)]
        bad = [i for i, c in enumerate(cls) if c]
        return BatchResult([c == 0 for c in cls], bad[0] if bad else None, cls)

    def tlock_open_rounds(self, sigs, us_per_round):
        from drand_amd.engine import TlockRoundsResult
        self.calls.append("tlock_open_rounds")
        ok, cls, gt, sig_class = [], [], [], []
        for sig, run in zip(sigs, us_per_round):
            sig = bytes(sig)
            sc = self.c.g2_decode_class(sig)
            sig_class.append(sc)
            if sc == 0 and sig not in self.bases:
                self.bases[sig] = T.gt_base(O.g2_decompress(sig))
            for u in run:
                c = T.g1_class(u) or (REJ_TLOCK_SIG if sc else 0)
                cls.append(c)
                ok.append(c == 0)
                gt.append(T.encode_gt(T.gt_pow(self.bases[sig], self.scalars[bytes(u)])) if c == 0 else None)
        return TlockRoundsResult(ok, cls, gt, sig_class)
