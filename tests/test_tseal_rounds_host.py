"""The timelock sealing to many rounds on the host build (tools/opcount tsealr: drand_amd/csrc/tsealr.h
compiled with -DBLS_HOST, the key table, the fixed-base walk and the single-pair Miller passes as
k_tsealr.hip runs them) against the Python oracle and the tool's plain second implementation, its
Fp-product counts against the frozen ones and against the two-pair passes', the round trip through
tools/opcount tlock, the entry points' size arithmetic (tools/hosttest.cpp, stand-alone under
ASan+UBSan), and callers.timelock_seal_rounds on a stand-in engine backed by the oracle. No GPU.

One oracle pairing per distinct round, three in this module.
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
from tests.support import tsealr_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
ROUNDS = (7, 8, 2 ** 64 - 1)
PK_PT = O.sk_to_pk(SK)
PK = O.g1_compress(PK_PT)
EDGE_ROUNDS = [ROUNDS[i % 3] for i in range(len(S.EDGE))]


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


@pytest.fixture(scope="module")
def want():
    return SR.RoundExpectations(PK_PT)  # the module's pairings, one per round of ROUNDS


def run_tsealr(binp, pk, rounds, scalars):
    r = subprocess.run([binp, "tsealr", pk.hex()],
                       input="".join("%d %s\n" % (rd, S.be32(k).hex()) for rd, k in zip(rounds, scalars)),
                       capture_output=True, text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


@pytest.fixture(scope="module")
def edge_run(opcount_bin):
    """One run of the tool over the edge scalars, the rounds cycling over ROUNDS; shared by the tests below."""
    return run_tsealr(opcount_bin, PK, EDGE_ROUNDS, S.EDGE)


def test_values_match_oracle(edge_run, want):
    rc, out = edge_run
    assert rc == 0
    for i, (rd, k) in enumerate(zip(EDGE_ROUNDS, S.EDGE)):
        ok, u, gt = want(rd, k)
        assert ok == (k not in S.REFUSED)
        assert (out["ok"][i], bytes.fromhex(out["u"][i]), bytes.fromhex(out["k"][i])) == (int(ok), u, gt), (i, rd, hex(k))
    one = S.EDGE.index(1)
    assert bytes.fromhex(out["k"][one]) == T.encode_gt(want.base(EDGE_ROUNDS[one]))  # K of scalar 1 is the round's base
    # the same scalar (mod r) under two rounds: one U, two K
    a, b = S.EDGE.index(1), S.EDGE.index(S.R + 1)
    assert EDGE_ROUNDS[a] != EDGE_ROUNDS[b] and out["u"][a] == out["u"][b] and out["k"][a] != out["k"][b]
    for k in S.REFUSED:
        i = S.EDGE.index(k)
        assert out["ok"][i] == 0 and bytes.fromhex(out["u"][i]) == bytes(48) and bytes.fromhex(out["k"][i]) == bytes(576)


def test_table_and_second_implementation(edge_run):
    """Every key-table entry equals jac_mul_scalar of pk (the tool's own check), the two-pair f pass with
    an inactive second pair gives the single-pair f, and jac_mul_scalar with miller_loop_multi<1> and the
    register final exponentiation give the staged path's bytes."""
    rc, out = edge_run
    assert rc == 0 and out["table_match"] is True and out["two_pair_match"] is True
    assert out["u_plain"] == out["u"] and out["k_plain"] == out["k"]


def test_round_trip_through_the_opening(opcount_bin, edge_run):
    """open(sigma_round, U_i) == K_i on the host build, per round: the prepared-table Miller loop of
    tools/opcount tlock against the per-item single-pair pairing of tools/opcount tsealr."""
    _, out = edge_run
    for rd in ROUNDS:
        acc = [i for i, k in enumerate(S.EDGE) if k not in S.REFUSED and EDGE_ROUNDS[i] == rd]
        assert acc
        sig = C.sign(SK, O.message_v2(rd))
        r = subprocess.run([opcount_bin, "tlock", sig.hex()], input="".join(out["u"][i] + "\n" for i in acc),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        opened = json.loads(r.stdout)
        assert opened["class"] == [0] * len(acc)
        assert opened["e"] == [out["k"][i] for i in acc], rd


def test_op_counts(opcount_bin):
    """The counts of one item with the full-width scalar equal the frozen ones; a single pair's lines cost
    exactly half of the two-pair lines, and its f pass strictly less than the two-pair f pass."""
    rc, out = run_tsealr(opcount_bin, PK, [ROUNDS[0]], [S.FULL])
    assert rc == 0 and out["ok"] == [1]
    mine = json.load(open(os.path.join(ROOT, "profiles", "tsealr_opcount.json")))["fp_mul"]
    m = out["fp_mul"]
    print("tsealr fp_mul", m)
    assert m == mine, "profiles/tsealr_opcount.json is stale"
    assert m["lines1"] > 0 and 2 * m["lines1"] == m["lines2"]
    assert 0 < m["f1"] < m["f2"]
    assert 0 < m["p_fixed"] <= m["u_fixed"]  # the same walk; U pays its compression on top


def test_bad_key_is_refused(opcount_bin):
    for pk in list(T.bad_us().values()) + [b"\xc0" + bytes(47)]:
        r = subprocess.run([opcount_bin, "tsealr", pk.hex()], input="7 " + S.be32(1).hex() + "\n",
                           capture_output=True, text=True)
        out = json.loads(r.stdout)
        assert r.returncode == 1 and "u" not in out and (out["pk_class"] != 0 or out["pk_inf"] is True)


def test_size_arithmetic_asan():
    """hostlogic.h seal_rounds_fits / seal_rounds_layout in tools/hosttest.cpp (a stand-alone program under
    ASan+UBSan): the guard on a caller's n at both sides of its limit, and the S-staging layout of a pass
    (P table | scalars | rounds | U bytes | ok bytes, within 192 bytes per item)."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "hosttest-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "hosttest-asan"), "hostlogic"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["hostlogic"]["seal_rounds"]
    lim = (2 ** 64 - 1) // 576
    assert out["fits"] == [n <= lim for n in (0, 1, 1 << 20, lim, lim + 1, 2 ** 64 - 1)]
    assert out["fits"] == [True, True, True, True, False, False]

    def layout(c):
        o_sc = 96 * c
        o_rd = o_sc + 32 * c
        o_us = o_rd + 8 * c
        o_ok = o_us + 48 * c
        return [0, o_sc, o_rd, o_us, o_ok, o_ok + c, o_rd]
    assert out["layout"] == [layout(c) for c in (1, 64, 16384, 1 << 20)]


# ------------------------------------------------------------------ callers.timelock_seal_rounds, stand-in engine
MSGS = [b"", b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100))]
ITEMS = list(zip([7, 8, 7, 2 ** 64 - 1], MSGS))


def open_per_round(eng, items, cts, **kw):
    got = [None] * len(items)
    for rd in sorted({r for r, _ in items}):
        mine = [i for i, (r, _) in enumerate(items) if r == rd]
        sig = C.sign(SK, O.message_v2(rd))
        for i, m in zip(mine, callers.timelock_open(eng, rd, sig, [cts[i] for i in mine], callers.kdf_sha256_ctr, **kw)):
            got[i] = m
    return got


def test_timelock_seal_rounds_on_stand_in():
    eng = SR.OracleSealRoundsEngine(PK)
    ks = [3, 5, S.FULL, 11]
    cts = callers.timelock_seal_rounds(eng, ITEMS, callers.kdf_sha256_ctr, scalars=ks)
    assert eng.calls == ["tlock_seal_rounds"]
    assert [len(c) for _, c in cts] == [0, 1, 32, 100]
    # each item is what the one-round caller gives for its round and scalar
    for i, (rd, m) in enumerate(ITEMS):
        assert [cts[i]] == callers.timelock_seal(eng, rd, [m], callers.kdf_sha256_ctr, scalars=[ks[i]])
    assert cts[2] == T.encrypt(PK_PT, 7, MSGS[2], S.FULL, callers.kdf_sha256_ctr)  # the support encryptor
    assert open_per_round(eng, ITEMS, cts) == MSGS


def test_timelock_seal_rounds_draws_its_own_scalars():
    eng = SR.OracleSealRoundsEngine(PK)
    a = callers.timelock_seal_rounds(eng, ITEMS[:2], callers.kdf_sha256_ctr)
    b = callers.timelock_seal_rounds(eng, ITEMS[:2], callers.kdf_sha256_ctr)
    us = [u for u, _ in a + b]
    assert len(set(us)) == 4 and all(len(u) == 48 for u in us)
    assert all(0 < k < S.R for k in eng.scalars.values())
    assert open_per_round(eng, ITEMS[:2], a, verify=False) == MSGS[:2]


def test_timelock_seal_rounds_refuses_and_checks():
    eng = SR.OracleSealRoundsEngine(PK)
    for zero in S.REFUSED:
        with pytest.raises(ValueError):
            callers.timelock_seal_rounds(eng, ITEMS[:2], callers.kdf_sha256_ctr, scalars=[3, zero])
    with pytest.raises(ValueError):  # one scalar per item
        callers.timelock_seal_rounds(eng, ITEMS[:2], callers.kdf_sha256_ctr, scalars=[3])
    with pytest.raises(ValueError):  # a short KDF result
        callers.timelock_seal_rounds(eng, ITEMS[2:3], lambda gt, n: bytes(n - 1), scalars=[3])
