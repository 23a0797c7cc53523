"""The timelock sealing on the host build (tools/opcount tseal: drand_amd/csrc/tseal.h compiled with
-DBLS_HOST, the tables and the table walks as k_tseal.hip runs them) against the Python oracle, its
Fp-product counts against the frozen ones and against an opening's, the round trip through
tools/opcount tlock, and callers.timelock_seal on a stand-in engine backed by the oracle. No GPU.

Every expectation is a power of ONE oracle pairing, B = e(pk, H(MessageV2(round)))^3.
"""
import json
import os
import subprocess

import pytest

from drand_amd import callers
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import tlock_ref as T
from tests.support import tseal_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
ROUND = 7
PK_PT = O.sk_to_pk(SK)
PK = O.g1_compress(PK_PT)


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


@pytest.fixture(scope="module")
def want():
    return S.Expectations(S.kbase(PK_PT, ROUND))  # the module's one pairing


def run_tseal(binp, pk, round_, scalars):
    r = subprocess.run([binp, "tseal", pk.hex(), str(round_)], input="".join(S.be32(k).hex() + "\n" for k in scalars),
                       capture_output=True, text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


@pytest.fixture(scope="module")
def edge_run(opcount_bin):
    """One run of the tool over the edge scalars, shared by the tests below."""
    return run_tseal(opcount_bin, PK, ROUND, S.EDGE)


def test_values_match_oracle(edge_run, want):
    rc, out = edge_run
    assert rc == 0
    for i, k in enumerate(S.EDGE):
        ok, u, gt = want(k)
        assert ok == (k not in S.REFUSED)
        assert (out["ok"][i], bytes.fromhex(out["u"][i]), bytes.fromhex(out["k"][i])) == (int(ok), u, gt), (i, hex(k))
    one = S.EDGE.index(1)
    for k in (S.R + 1, 2 * S.R + 1):  # both == 1 (mod r): the bytes of scalar 1
        i = S.EDGE.index(k)
        assert (out["u"][i], out["k"][i]) == (out["u"][one], out["k"][one])
    assert bytes.fromhex(out["k"][one]) == T.encode_gt(want.base)  # K of scalar 1 is B itself
    for k in S.REFUSED:
        i = S.EDGE.index(k)
        assert out["ok"][i] == 0 and bytes.fromhex(out["u"][i]) == bytes(48) and bytes.fromhex(out["k"][i]) == bytes(576)


def test_tables_and_second_implementation(edge_run):
    """Every T1 entry equals jac_mul_scalar of the generator and every T2 entry a plain power of B (the
    tool's own check), and jac_mul_scalar / cyclotomic square-and-multiply give the table walks' bytes."""
    rc, out = edge_run
    assert rc == 0 and out["tables_match"] is True
    assert out["u_plain"] == out["u"] and out["k_plain"] == out["k"]


def test_op_counts(opcount_bin):
    """A seal runs no pairing per item: with the full-width scalar its two table walks cost less than
    their plain forms, and together less than an opening's f pass and final exponentiation."""
    rc, out = run_tseal(opcount_bin, PK, ROUND, [S.FULL])
    assert rc == 0 and out["ok"] == [1]
    mine = json.load(open(os.path.join(ROOT, "profiles", "tseal_opcount.json")))["fp_mul"]
    opening = json.load(open(os.path.join(ROOT, "profiles", "tlock_opcount.json")))["fp_mul"]
    m = out["fp_mul"]
    print("tseal fp_mul", m, "opening", opening)
    assert m == mine, "profiles/tseal_opcount.json is stale"
    assert 0 < m["u_fixed"] < m["u_plain"]
    assert 0 < m["gt_fixed"] < m["gt_plain"]
    assert m["u_fixed"] + m["gt_fixed"] < opening["tlock_f"] + opening["final_exp"]


def test_round_trip_through_the_opening(opcount_bin, edge_run):
    """open(sigma_round, U_i) == K_i on the host build: the Miller loop and final exponentiation of
    tools/opcount tlock against the Gt powers of tools/opcount tseal."""
    _, out = edge_run
    acc = [i for i, k in enumerate(S.EDGE) if k not in S.REFUSED]
    sig = C.sign(SK, O.message_v2(ROUND))
    r = subprocess.run([opcount_bin, "tlock", sig.hex()], input="".join(out["u"][i] + "\n" for i in acc),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    opened = json.loads(r.stdout)
    assert opened["class"] == [0] * len(acc)
    assert opened["e"] == [out["k"][i] for i in acc]


def test_bad_key_is_refused(opcount_bin):
    for pk in list(T.bad_us().values()) + [b"\xc0" + bytes(47)]:
        r = subprocess.run([opcount_bin, "tseal", pk.hex(), str(ROUND)], input=S.be32(1).hex() + "\n",
                           capture_output=True, text=True)
        out = json.loads(r.stdout)
        assert r.returncode == 1 and "u" not in out and (out["pk_class"] != 0 or out["pk_inf"] is True)


# ------------------------------------------------------------------ callers.timelock_seal, stand-in engine
MSGS = [b"", b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100))]


def test_timelock_seal_on_stand_in():
    eng = S.OracleSealEngine(PK)
    ks = [3, 5, S.FULL, 11]
    cts = callers.timelock_seal(eng, ROUND, MSGS, callers.kdf_sha256_ctr, scalars=ks)
    assert eng.calls == ["tlock_seal"]
    assert [len(c) for _, c in cts] == [0, 1, 32, 100]
    # the support encryptor, for a given scalar
    assert cts[2] == T.encrypt(PK_PT, ROUND, MSGS[2], S.FULL, callers.kdf_sha256_ctr)
    assert cts[3] == T.encrypt(PK_PT, ROUND, MSGS[3], 11, callers.kdf_sha256_ctr)
    # and back through the opening
    sig = C.sign(SK, O.message_v2(ROUND))
    assert callers.timelock_open(eng, ROUND, sig, cts, callers.kdf_sha256_ctr) == MSGS


def test_timelock_seal_draws_its_own_scalars():
    eng = S.OracleSealEngine(PK)
    a = callers.timelock_seal(eng, ROUND, MSGS[:2], callers.kdf_sha256_ctr)
    b = callers.timelock_seal(eng, ROUND, MSGS[:2], callers.kdf_sha256_ctr)
    us = [u for u, _ in a + b]
    assert len(set(us)) == 4 and all(len(u) == 48 for u in us)
    assert all(0 < k < S.R for k in eng.scalars.values())
    sig = C.sign(SK, O.message_v2(ROUND))
    assert callers.timelock_open(eng, ROUND, sig, a, callers.kdf_sha256_ctr, verify=False) == MSGS[:2]


def test_timelock_seal_refuses_and_checks():
    eng = S.OracleSealEngine(PK)
    for zero in S.REFUSED:
        with pytest.raises(ValueError):
            callers.timelock_seal(eng, ROUND, MSGS[:2], callers.kdf_sha256_ctr, scalars=[3, zero])
    with pytest.raises(ValueError):  # one scalar per message
        callers.timelock_seal(eng, ROUND, MSGS[:2], callers.kdf_sha256_ctr, scalars=[3])
    with pytest.raises(ValueError):  # a short KDF result
        callers.timelock_seal(eng, ROUND, MSGS[2:3], lambda gt, n: bytes(n - 1), scalars=[3])
