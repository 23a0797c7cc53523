"""Shared expectations of the tests of timelock sealing to many rounds, from the Python oracle and
tests/support/tseal_ref.py alone: TEST INFRASTRUCTURE ONLY.

Item i seals scalar k_i to its own round_i: U = (k mod r) * G1 and K = B_round^(k mod r) with
B_round = e(pk, H(MessageV2(round)))^3. One oracle pairing per DISTINCT round (about 0.65 s each in pure
Python: a test keeps to at most 4 of them); every other expectation is a power of one of them.
"""
from __future__ import annotations

from oracle import bls12381 as O
from tests.support import tseal_ref as S


class RoundExpectations:
    """(ok, U48, K576) of (round, k) under one key point; one S.Expectations, so one pairing, per
    distinct round, shared by every test that holds the object."""

    def __init__(self, pk_pt):
        self.pk_pt = pk_pt
        self.per_round = {}

    def base(self, round_):
        return self.of(round_).base

    def of(self, round_):
        if round_ not in self.per_round:
            self.per_round[round_] = S.Expectations(S.kbase(self.pk_pt, round_))
        return self.per_round[round_]

    def __call__(self, round_, k):
        return self.of(round_)(k)


class OracleSealRoundsEngine(S.OracleSealEngine):
    """OracleSealEngine with Engine.tlock_seal_rounds beside tlock_seal, answered by the oracle: one
    pairing per distinct (key, round) of a call; every sealed U is remembered with its scalar so that
    tlock_open can open it."""

    def tlock_seal_rounds(self, rounds, scalars, pk48=None):
        from drand_amd.engine import TsealResult
        self.calls.append("tlock_seal_rounds")
        rounds, scalars = list(rounds), list(scalars)
        assert len(rounds) == len(scalars)
        pk = self.pk if pk48 is None else bytes(pk48)
        oks, us, gts = [], [], []
        for round_, k in zip(rounds, scalars):
            key = (pk, int(round_))
            if key not in self.kbases:
                self.kbases[key] = S.kbase(O.g1_decompress(pk), int(round_))
            k = int.from_bytes(k, "big") if isinstance(k, (bytes, bytearray)) else int(k)
            ok, u, gt = S.expect(self.kbases[key], k)
            oks.append(ok)
            us.append(u if ok else None)
            gts.append(gt if ok else None)
            if ok:
                self.scalars[u] = k % S.R
        return TsealResult(oks, us, gts)
