"""The randomized batch verification's combination stage on the host build (tools/opcount rlc:
drand_amd/csrc/rlc.h compiled with -DBLS_HOST, lanes and groups laid out as k_rlc.hip lays them out)
against the Python oracle: every group's A = sum r_i H_i and B = sum r_i sigma_i with
r_i = first 8 bytes of SHA-256(seed || BE64(i)), and the stage's Fp-product count per beacon against
the pairing stages it replaces. No GPU.

Also the CPU twin of the callers test of tests/test_gpu_rlc.py: VerifyingClient and sync_chain with
fast=True against a stand-in engine defined here.
"""
import hashlib
import json
import os
import subprocess

import pytest

from oracle import bls12381 as O
from oracle import c_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes(range(7, 39))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
G = 8
N = 19  # two full groups and a ragged one


def rlc_scalar(seed, i):
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, "big")).digest()[:8], "big")


def oracle_sums(seed, group, hs, sigs, skip=()):
    """([A_g], [B_g]) compressed; hs / sigs are oracle points (None = infinity), skip = indices left
    out of both sums (decode rejects)."""
    a, b = [], []
    for lo in range(0, len(hs), group):
        sa = sb = None
        for i in range(lo, min(lo + group, len(hs))):
            if i in skip:
                continue
            r = rlc_scalar(seed, i)
            if hs[i] is not None:
                sa = O.g2_add(sa, O.g2_mul(hs[i], r))
            if sigs[i] is not None:
                sb = O.g2_add(sb, O.g2_mul(sigs[i], r))
        a.append(O.g2_compress(sa))
        b.append(O.g2_compress(sb))
    return a, b


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


@pytest.fixture(scope="module")
def signed():
    msgs = [b"rlc host item %d" % i for i in range(N)]
    return msgs, [C.sign(SK, m) for m in msgs]


def run_rlc(binp, seed, group, msgs, sigs):
    lines = "".join("%s %s\n" % (m.hex(), s.hex()) for m, s in zip(msgs, sigs))
    r = subprocess.run([binp, "rlc", seed.hex(), str(group)], input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def check(binp, msgs, sigs):
    out = run_rlc(binp, SEED, G, msgs, sigs)
    # (the oracle's own [r]P subgroup test is skipped: H comes from its hash, sigma from its sign)
    hs = [O.g2_decompress(C.hash_to_g2(m), check_subgroup=False) for m in msgs]
    ss = [O.g2_decompress(s, check_subgroup=False) for s in sigs]
    want_a, want_b = oracle_sums(SEED, G, hs, ss)
    assert out["items"] == len(msgs) and out["groups"] == len(want_a)
    assert [bytes.fromhex(x) for x in out["a"]] == want_a
    assert [bytes.fromhex(x) for x in out["b"]] == want_b
    return out


def test_sums_match_oracle_and_cost_is_a_quarter(opcount_bin, signed):
    msgs, sigs = signed
    out = check(opcount_bin, msgs, sigs)
    # the pairing stages this replaces: the Miller loop's frozen count, and the final exponentiation
    # scaled from it by the measured stage times (188 ms and 135 ms per 1M beacons)
    miller = json.load(open(os.path.join(ROOT, "profiles", "opcount.json")))["fp_mul"]["miller"]
    pairing = miller + miller * 135 / 188
    print("rlc fp_mul per item %.1f, Miller + final exponentiation %.1f" % (out["fp_mul_per_item"], pairing))
    assert out["fp_mul_per_item"] <= pairing / 4


def test_repeated_and_negated_signatures(opcount_bin, signed):
    """sigma_j = sigma_i and sigma_k = -sigma_i on consecutive items: the running sum meets P == Q and
    P == -Q, so the complete addition's exceptional branches run."""
    msgs, sigs = signed
    sigs = list(sigs)
    neg = bytearray(sigs[1])
    neg[0] ^= 0x20
    sigs[2] = sigs[1]
    sigs[3] = bytes(neg)
    # and at the head of a lane, where the accumulator still is the first point alone
    sigs[9] = sigs[8]
    neg = bytearray(sigs[16])
    neg[0] ^= 0x20
    sigs[17] = bytes(neg)
    check(opcount_bin, msgs, sigs)


# ------------------------------------------------------------------ callers, CPU twin
class StandInEngine:
    """Just enough of Engine for the callers: chained ranges answered by the C oracle, whichever of the
    two methods is asked. Records which method served each call."""

    def __init__(self):
        self.calls = []

    def set_public_key(self, pk):
        self.pk = bytes(pk)

    def _chained(self, name, first_round, prev0, sigs):
        from drand_amd.engine import BatchResult
        self.calls.append(name)
        cls = C.verify_chained(self.pk, first_round, bytes(prev0), b"".join(sigs))
        bad = [i for i, c in enumerate(cls) if c]
        return BatchResult([c == 0 for c in cls], first_round + bad[0] if bad else None, cls)

    def verify_chained(self, first_round, prev0, sigs):
        return self._chained("verify_chained", first_round, prev0, sigs)

    def verify_chained_rlc(self, first_round, prev0, sigs):
        return self._chained("verify_chained_rlc", first_round, prev0, sigs)


def callers_outcomes(make_engine, golden, fast):
    """What VerifyingClient and sync_chain do over the golden chain, clean and with round 9 corrupted:
    results and errors in a comparable form (shared with tests/test_gpu_rlc.py)."""
    from drand_amd.callers import Beacon, ChainInfo, RandomData, VerifyError, VerifyingClient, sync_chain
    ch = golden["chained"]
    pk, seed = bytes.fromhex(ch["pk"]), bytes.fromhex(ch["genesis_seed"])
    bs = [Beacon(bytes.fromhex(b["prev"]), b["round"], bytes.fromhex(b["sig"])) for b in ch["beacons"]]
    out = []
    for tamper in ({}, {9: bs[7].signature}):
        def get(r):
            b = bs[r - 1]
            return RandomData(round=r, signature=tamper.get(r, b.signature), previous_signature=b.previous_sig)
        eng = make_engine()
        vc = VerifyingClient(eng, ChainInfo(pk, seed), get, chunk=16, fast=fast,
                             point_of_trust=RandomData(round=1, signature=bs[0].signature,
                                                       previous_signature=bs[0].previous_sig))
        r = RandomData(round=24, signature=bs[23].signature)
        try:
            vc.verify(r)
            out.append(("verified", r.randomness, vc.point_of_trust.round))
        except VerifyError as e:
            out.append(("VerifyError", e.round, str(e), vc.point_of_trust.round))
        served = [Beacon(b.previous_sig, b.round, tamper.get(b.round, b.signature)) for b in bs]
        put = []
        o = sync_chain(eng, pk, Beacon(b"", 0, seed), iter(served), 24, put.append, chunk=16, fast=fast)
        out.append((o.finished, o.stored, o.reason, o.bad_round, o.last.round, [b.round for b in put]))
    return out


def test_callers_fast_matches_default_on_stand_in(golden):
    engines = {False: [], True: []}

    def make(fast):
        def f():
            engines[fast].append(StandInEngine())
            return engines[fast][-1]
        return f
    want = callers_outcomes(make(False), golden, False)
    got = callers_outcomes(make(True), golden, True)
    assert got == want
    assert want[0][0] == "verified" and want[2][0] == "VerifyError" and want[2][1] == 9
    # the walked and the linked ranges went to the method asked for (the lone requested round of
    # VerifyingClient.verify always takes the exact check)
    assert {c for e in engines[False] for c in e.calls} == {"verify_chained"}
    for e in engines[True]:
        assert e.calls.count("verify_chained_rlc") >= 2 and e.calls.count("verify_chained") <= 1
