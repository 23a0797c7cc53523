"""The timelock opening on the host build (tools/opcount tlock: drand_amd/csrc/tlock.h compiled with
-DBLS_HOST, the prepared line table and the f pass as k_tlock.hip runs them) against the Python oracle,
its Fp-product counts against the frozen two-pair Miller count, and callers.timelock_open on a stand-in
engine backed by the oracle. No GPU.

The oracle's reduced pairing is e = f^((p^12 - 1)/r); the engine returns its cube (the hard part
(x-1)^2 (x+p) (x^2+p^2-1) + 3 = 3 (p^4 - p^2 + 1)/r), so every expectation is f12_pow(pairing, 3).
"""
import json
import os
import subprocess

import pytest

from drand_amd import callers
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import tlock_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
ROUND = 7
R1 = 0x5B1E7C0FFEE0DDBA11AD5EED0123456789ABCDEF0FEDCBA9876543210F1E2D3C % O.R
R2 = (O.R - 0x1234567) % O.R  # full width, top bits set


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


@pytest.fixture(scope="module")
def sig():
    return C.sign(SK, O.message_v2(ROUND))


@pytest.fixture(scope="module")
def base(sig):
    return T.gt_base(O.g2_decompress(sig, check_subgroup=False))  # ONE oracle pairing for the module


def run_tlock(binp, sig, us):
    r = subprocess.run([binp, "tlock", sig.hex()], input="".join(u.hex() + "\n" for u in us), capture_output=True,
                       text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


def test_identity_lambda_is_three_times_the_oracle_hard_part():
    x = O.X
    assert (x - 1) ** 2 * (x + O.P) * (x * x + O.P * O.P - 1) + 3 == 3 * O.FINAL_EXP_HARD


def test_values_match_oracle(opcount_bin, sig, base):
    """generator, two full-width multiples, infinity: E = f12_pow(pairing(U, sigma), 3), encoded per the
    header. The generator's value is the oracle pairing itself; the multiples follow by bilinearity
    (checked once against a direct oracle pairing for R1)."""
    us = [T.u_of(1), T.u_of(R1), T.u_of(R2), T.u_of(0)]
    rc, out = run_tlock(opcount_bin, sig, us)
    assert rc == 0 and out["sig_class"] == 0 and out["class"] == [0, 0, 0, 0]
    want = [T.encode_gt(base), T.encode_gt(T.gt_pow(base, R1)), T.encode_gt(T.gt_pow(base, R2)), T.GT_ONE]
    assert [bytes.fromhex(e) for e in out["e"]] == want
    direct = O.f12_pow(O.pairing(O.g1_decompress(us[1]), O.g2_decompress(sig, check_subgroup=False)), 3)
    assert T.encode_gt(direct) == want[1]
    assert T.encode_gt(O.F12_ONE) == T.GT_ONE


def test_prepared_lines_equal_the_miller_steps(opcount_bin, sig):
    """The tool compares, for every U, each of the 68 table lines times (xU, yU) with the line
    miller_lines emits for the same pair, and the f pass with miller_loop_multi<1>."""
    rc, out = run_tlock(opcount_bin, sig, [T.u_of(1), T.u_of(R1), T.u_of(R2)])
    assert rc == 0 and out["lines_match"] is True


def test_sigma_at_infinity_gives_ones(opcount_bin):
    inf = b"\xc0" + bytes(95)
    rc, out = run_tlock(opcount_bin, inf, [T.u_of(1), T.u_of(R1), T.u_of(0)])
    assert rc == 0 and out["sig_inf"] is True
    assert [bytes.fromhex(e) for e in out["e"]] == [T.GT_ONE] * 3


def test_rejected_u_and_sigma(opcount_bin, sig):
    bad = T.bad_us()
    rc, out = run_tlock(opcount_bin, sig, [bad[c] for c in sorted(bad)] + [T.u_of(1)])
    assert rc == 0 and out["class"] == sorted(bad) + [0]
    assert out["e"][:5] == [None] * 5 and out["e"][5] is not None
    for c, s in T.bad_sigs(sig).items():
        rc, out = run_tlock(opcount_bin, s, [T.u_of(1)])
        assert rc == 1 and out == {"sig_class": c}


def test_f_pass_is_cheaper_than_the_two_pair_miller_loop(opcount_bin, sig):
    rc, out = run_tlock(opcount_bin, sig, [T.u_of(R1)])
    frozen = json.load(open(os.path.join(ROOT, "profiles", "opcount.json")))["fp_mul"]
    mine = json.load(open(os.path.join(ROOT, "profiles", "tlock_opcount.json")))["fp_mul"]
    print("tlock fp_mul", out["fp_mul"], "frozen miller", frozen["miller"])
    assert out["fp_mul"] == mine, "profiles/tlock_opcount.json is stale"
    assert 0 < out["fp_mul"]["tlock_f"] < frozen["miller"]
    assert out["fp_mul"]["final_exp"] == frozen["final_exp"]


# ------------------------------------------------------------------ callers.timelock_open, stand-in engine
def test_timelock_open_round_trips_on_stand_in(sig):
    pk_pt = O.sk_to_pk(SK)
    pk = O.g1_compress(pk_pt)
    msgs = [b"", b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100))]
    rs = [3, 5, R1, 11]
    # one oracle pairing: K_i = (e(pk, H)^3)^r_i
    kbase = O.f12_pow(O.pairing(pk_pt, O.hash_to_g2(O.message_v2(ROUND))), 3)
    cts = []
    for m, r in zip(msgs, rs):
        ks = callers.kdf_sha256_ctr(T.encode_gt(T.gt_pow(kbase, r)), len(m))
        cts.append((T.u_of(r), bytes(a ^ b for a, b in zip(m, ks))))
    bad_u = T.bad_us()[O.REJ_NOT_ON_CURVE]
    cts.append((bad_u, b"whatever"))
    scalars = {T.u_of(r): r for r in rs}
    eng = T.OracleTlockEngine(pk, scalars)
    got = callers.timelock_open(eng, ROUND, sig, cts, callers.kdf_sha256_ctr)
    assert got == msgs + [None]
    assert eng.calls == ["verify_unchained", "tlock_open"]
    # the beacon of another round is refused before anything is opened
    eng.calls.clear()
    with pytest.raises(callers.VerifyError) as ei:
        callers.timelock_open(eng, ROUND + 1, sig, cts, callers.kdf_sha256_ctr)
    assert ei.value.round == ROUND + 1 and eng.calls == ["verify_unchained"]
    # the kdf is the caller's: another one gives other bytes, verify=False skips the beacon check
    eng.calls.clear()
    other = callers.timelock_open(eng, ROUND, sig, cts[:4], T.sha_kdf, verify=False)
    assert eng.calls == ["tlock_open"] and other[0] == b"" and other[3] != msgs[3]


def test_support_consecutive_points():
    """The GPU tests' batch-inverted (i + 1) * G1 table against the oracle's scalar multiplication."""
    us = T.consecutive_us(70)
    assert us == [T.u_of(i + 1) for i in range(70)]
    assert T.consecutive_us(1) == [T.u_of(1)]


def test_kdf_sha256_ctr_blocks():
    import hashlib
    gt = bytes(range(256)) * 2 + bytes(64)
    assert callers.kdf_sha256_ctr(gt, 0) == b""
    want = hashlib.sha256(gt + bytes(4)).digest() + hashlib.sha256(gt + b"\x00\x00\x00\x01").digest()
    assert callers.kdf_sha256_ctr(gt, 40) == want[:40]
