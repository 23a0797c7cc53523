"""The timelock opening across many rounds on the host build (tools/opcount tlockr: drand_amd/csrc/tlockr.h
compiled with -DBLS_HOST -- the host's plan, the many-signature prepare into the word-major table and both
forms of the f pass as k_tlockr.hip runs them) against the Python oracle by bilinearity, the plan rule and
the entry points' size arithmetic (tools/hosttest.cpp, stand-alone under ASan+UBSan), and
callers.timelock_open_rounds on a stand-in engine backed by the oracle. No GPU.

One oracle pairing per distinct decodable signature: two in the value tests, three in the stand-in tests.
"""
import json
import os
import subprocess

import pytest

from drand_amd import callers
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import tlock_ref as T
from tests.support import tlockr_ref as TR
from tests.support import tseal_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
PK_PT = O.sk_to_pk(SK)
PK = O.g1_compress(PK_PT)
SIG_INF = b"\xc0" + bytes(95)
ALL_MIXED = 2 ** 64 - 1


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


def run_tlockr(binp, cap, dense_min, sigs, runs):
    args = [binp, "tlockr", str(cap), str(dense_min)]
    for s, run in zip(sigs, runs):
        args += [s.hex(), str(len(run))]
    r = subprocess.run(args, input="".join(u.hex() + "\n" for run in runs for u in run), capture_output=True, text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


@pytest.fixture(scope="module")
def case():
    """(sigs, runs of U, expected class and encoding per item, expected sig_class): two decodable
    signatures (two pairings), one that is not on the curve, the point at infinity, and a round without
    items; rejected U values and U at infinity inside the runs."""
    s7, s8 = C.sign(SK, O.message_v2(7)), C.sign(SK, O.message_v2(8))
    bad_sig = T.bad_sigs(s7)[O.REJ_NOT_ON_CURVE]
    bad_u = T.bad_us()
    bases = TR.Bases()
    long_run = T.consecutive_us(66)
    sigs = [s7, bad_sig, SIG_INF, s8, s8, s7]
    runs = [[T.u_of(2), T.u_of(0), bad_u[5]], [T.u_of(3), bad_u[6]], [T.u_of(4), T.u_of(0)], [], long_run, [T.u_of(7)]]
    want = [(0, TR.expected(bases, s7, [2])[0]), (0, T.GT_ONE), (5, None),
            (TR.REJ_TLOCK_SIG, None), (6, None),
            (0, T.GT_ONE), (0, T.GT_ONE)]
    want += [(0, e) for e in T.running_gts(bases(s8), 66)]
    want += [(0, TR.expected(bases, s7, [7])[0])]
    return sigs, runs, want, [0, O.REJ_NOT_ON_CURVE, 0, 0, 0, 0]


@pytest.mark.parametrize("cap,dense_min", [(1024, 1), (1024, 64), (1024, ALL_MIXED), (64, 64), (7, 2)])
def test_values_match_oracle_in_every_form(opcount_bin, case, cap, dense_min):
    """The same classes and bytes whatever the tiles: all uniform, the default split, all mixed, and passes
    of 64 and of 7 items that cut the long run (prepared again in every pass that touches it)."""
    sigs, runs, want, sig_class = case
    rc, out = run_tlockr(opcount_bin, cap, dense_min, sigs, runs)
    assert rc == 0 and out["forms_match"] is True
    assert out["sig_class"] == sig_class
    assert out["class"] == [c for c, _ in want]
    assert [None if e is None else bytes.fromhex(e) for e in out["e"]] == [e for _, e in want]
    assert out["tiles"] == [p[3] for p in TR.plan([len(r) for r in runs], cap, dense_min)]
    forms = {t[2] == TR.MIXED for tiles in out["tiles"] for t in tiles}
    # at a cap of 64 no part of a run reaches 64 items inside a pass
    assert forms == {(1024, 1): {False}, (1024, 64): {False, True}, (1024, ALL_MIXED): {True}, (64, 64): {True},
                     (7, 2): {False, True}}[(cap, dense_min)]


def test_sum_mismatch_is_refused(opcount_bin, case):
    sigs, runs, _, _ = case
    args = [opcount_bin, "tlockr", "1024", "64", sigs[0].hex(), "2", sigs[3].hex(), "2"]
    r = subprocess.run(args, input="".join(u.hex() + "\n" for u in runs[0]), capture_output=True, text=True)
    assert r.returncode == 1 and json.loads(r.stdout) == {"einval": True}


# ------------------------------------------------------------------ the plan rule, stand-alone under ASan+UBSan
RUNS = [0, 1, 63, 0, 64, 65, 129, 0]
PLAN_CASES = [(RUNS, 1024, 1), (RUNS, 1024, 64), (RUNS, 1024, ALL_MIXED), ([100, 60, 3], 128, 64), ([0, 0, 0], 64, 64),
              ([200], 64, 64), ([1, 1, 1, 1, 1], 64, 2)]
M = TR.MIXED
PLAN_WANT = [
    # dense_min 1: every run its own uniform tiles
    [[0, 322, [1, 2, 4, 5, 6], [[0, 1, 0], [1, 63, 1], [64, 64, 2], [128, 64, 3], [192, 1, 3], [193, 64, 4], [257, 64, 4],
                                [321, 1, 4]]]],
    # dense_min 64: the runs of 1 and 63 share one mixed tile; 64, 65 and 129 are dense
    [[0, 322, [1, 2, 4, 5, 6], [[0, 64, M], [64, 64, 2], [128, 64, 3], [192, 1, 3], [193, 64, 4], [257, 64, 4], [321, 1, 4]]]],
    # SIZE_MAX: consecutive items in tiles of 64 whatever their rounds
    [[0, 322, [1, 2, 4, 5, 6], [[0, 64, M], [64, 64, M], [128, 64, M], [192, 64, M], [256, 64, M], [320, 2, M]]]],
    # a run cut by the pass boundary: 28 of round 1's 60 items end pass 0, 32 start pass 1, both short
    [[0, 128, [0, 1], [[0, 64, 0], [64, 36, 0], [100, 28, M]]], [128, 35, [1, 2], [[0, 35, M]]]],
    [],
    # one run over four passes: its last 8 items are a short part
    [[0, 64, [0], [[0, 64, 0]]], [64, 64, [0], [[0, 64, 0]]], [128, 64, [0], [[0, 64, 0]]], [192, 8, [0], [[0, 8, M]]]],
    [[0, 5, [0, 1, 2, 3, 4], [[0, 5, M]]]],
]


def test_plan_rule_asan():
    """hostlogic.h open_rounds_fits / open_rounds_next_pass in tools/hosttest.cpp hostlogic (a stand-alone
    program under ASan+UBSan, which itself checks that every item is covered exactly once by a tile of its
    own signature): zero counts, runs of 1, 63, 64, 65 and 129, dense_min 1 / 64 / SIZE_MAX, runs cut by a
    pass boundary; a sum that differs from n, a sum that wraps and an n whose byte count overflows are
    refused. The expected tile lists are restated here and agree with the restated rule."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "hosttest-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "hosttest-asan"), "hostlogic"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["hostlogic"]["open_rounds"]
    lim = (2 ** 64 - 1) // 576
    fits = [([], 0), ([1, 2, 3], 6), ([1, 2, 3], 5), ([1, 2, 3], 7), ([0, 0], 0), ([2 ** 64 - 1, 2], 1), ([lim + 1], lim + 1),
            ([], 1), ([4, 2 ** 64 - 4, 4], 4)]
    assert out["fits"] == [sum(c) == n and n <= lim for c, n in fits]
    assert out["fits"] == [True, True, False, False, True, False, False, False, False]
    assert out["plans"] == PLAN_WANT
    assert [TR.plan(c, cap, d) for c, cap, d in PLAN_CASES] == PLAN_WANT
    for (counts, cap, _), passes in zip(PLAN_CASES, PLAN_WANT):
        seen = [0] * sum(counts)
        for base, cnt, sig_j, tiles in passes:
            assert 1 <= cnt <= cap and len(sig_j) <= cnt
            for first, length, _ in tiles:
                assert 1 <= length <= 64 and first + length <= cnt
                for i in range(base + first, base + first + length):
                    seen[i] += 1
        assert seen == [1] * sum(counts)


# ------------------------------------------------------------------ callers.timelock_open_rounds, stand-in engine
MSGS = [b"", b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100))]
SEALED_TO = [7, 8, 7, 2 ** 64 - 1]
KS = [3, 5, S.FULL, 11]


@pytest.fixture(scope="module")
def sealed():
    """(engine, rounds argument, messages per round): four messages sealed to three rounds by the support
    sealer (one pairing per round); a ciphertext with a wrong-length U and one whose U does not decode ride
    along in round 8. The engine knows every sealed U's scalar."""
    kb = {r: S.kbase(PK_PT, r) for r in sorted(set(SEALED_TO))}
    scalars, per_round = {}, {r: [] for r in kb}
    for r, m, k in zip(SEALED_TO, MSGS, KS):
        _, u, gt = S.expect(kb[r], k)
        scalars[u] = k % S.R
        per_round[r].append(((u, bytes(a ^ b for a, b in zip(m, callers.kdf_sha256_ctr(gt, len(m))))), m))
    per_round[8] += [((b"\x01" * 47, b"short U"), None), ((T.bad_us()[4], b"no such point"), None)]
    eng = TR.OracleOpenRoundsEngine(PK, scalars)
    for r, b in kb.items():  # e(G1, s H) = e(pk, H): the sealer's bases are the opener's
        eng.bases[C.sign(SK, O.message_v2(r))] = b
    rounds = [(r, C.sign(SK, O.message_v2(r)), [ct for ct, _ in per_round[r]]) for r in kb]
    return eng, rounds, [[m for _, m in per_round[r]] for r in kb]


def test_timelock_open_rounds_on_stand_in(sealed):
    eng, rounds, msgs = sealed
    eng.calls.clear()
    got = callers.timelock_open_rounds(eng, rounds, callers.kdf_sha256_ctr)
    assert eng.calls == ["verify_unchained", "tlock_open_rounds"]
    assert got == msgs and got == [[MSGS[0], MSGS[2]], [MSGS[1], None, None], [MSGS[3]]]
    # each round is what the one-round caller gives
    for (r, sig, cts), want in zip(rounds, got):
        assert callers.timelock_open(eng, r, sig, cts, callers.kdf_sha256_ctr) == want
    assert callers.timelock_open_rounds(eng, [], callers.kdf_sha256_ctr) == []


def test_timelock_open_rounds_refuses_a_swapped_signature(sealed):
    eng, rounds, msgs = sealed
    swapped = [rounds[0], (rounds[1][0], rounds[2][1], rounds[1][2]), (rounds[2][0], rounds[1][1], rounds[2][2])]
    eng.calls.clear()
    with pytest.raises(callers.VerifyError) as ei:
        callers.timelock_open_rounds(eng, swapped, callers.kdf_sha256_ctr)
    assert eng.calls == ["verify_unchained"]  # nothing was opened
    assert ei.value.round == rounds[1][0]  # the first rejected round
    with pytest.raises(callers.VerifyError):
        callers.timelock_open_rounds(eng, [(7, b"\x00" * 95, [])], callers.kdf_sha256_ctr)


def test_timelock_open_rounds_without_verification(sealed):
    eng, rounds, msgs = sealed
    eng.calls.clear()
    assert callers.timelock_open_rounds(eng, rounds, callers.kdf_sha256_ctr, verify=False) == msgs
    assert eng.calls == ["tlock_open_rounds"]
    # the neighbouring round's signature opens to other bytes of the same lengths, silently
    swapped = [(rounds[0][0], rounds[1][1], rounds[0][2])]
    wrong = callers.timelock_open_rounds(eng, swapped, callers.kdf_sha256_ctr, verify=False)
    assert [len(w) for w in wrong[0]] == [len(m) for m in msgs[0]] and wrong[0][1] != msgs[0][1]
    # a signature that does not decode opens nothing; the other rounds are unaffected
    bad = T.bad_sigs(rounds[0][1])[O.REJ_FLAG]
    got = callers.timelock_open_rounds(eng, [(rounds[0][0], bad, rounds[0][2]), rounds[2]], callers.kdf_sha256_ctr,
                                       verify=False)
    assert got == [[None, None], msgs[2]]
    with pytest.raises(ValueError):  # a short KDF result
        callers.timelock_open_rounds(eng, rounds[:1], lambda gt, n: bytes(max(n - 1, 0)), verify=False)
