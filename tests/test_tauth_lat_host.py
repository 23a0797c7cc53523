"""The authenticated timelock items of the latency engine (drand_amd/csrc/wauth.h: gt_midstate, auth_walk_team,
auth_open_item / auth_open_team, auth_seal_item / auth_seal_team) compiled for the host with wv.h's lane
emulation (tools/wvtest gtmid / awalk / tawalk / aopen / taopen / aseal / taseal) and checked on the CPU.

Expected bytes never come from the code under test: tests/support/tauth_ref.py (hashlib and Python integers)
over ONE oracle pairing for the module, the base of the golden chain's round 7 under its key. Tampered
ciphertexts are ordinary data to the items. The lane emulation is slow, so the item counts are the issue's.
The team commands also abort if a workgroup leaves seed-derived values in its LDS slots, and every command
guards its output bytes on both sides."""
import hashlib
import os
import subprocess

import pytest

from oracle import bls12381 as O
from tests.support import tauth_ref as A
from tests.support import tlock_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# WVTEST_TARGET=wvtest-asan runs the module on the ASan+UBSan build, as tests/test_tseal_lat_host.py does
TARGET = os.environ.get("WVTEST_TARGET", "wvtest")
BIN = os.path.join(ROOT, "tools", TARGET)

R = O.R
ROUND = 7
AUTH = A.REJ_TLOCK_AUTH
WIDE = 0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD % R
# the PLAIN scalars of tests/test_tseal_lat_host.py, then two that leave most waves' partial sums at infinity
PLAIN = [1, 2, 15, 16 ** 63, 16 ** 63 - 1, R - 1, WIDE]
SPARSE = [16 ** 8, 16 ** 56 + 16 ** 7]
INF_U = b"\xc0" + bytes(47)
INF_SIG = b"\xc0" + bytes(95)


@pytest.fixture(scope="module")
def wvtest():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), TARGET], check=True, capture_output=True)
    return BIN


def run(binary, cmd, lines):
    r = subprocess.run([binary, cmd], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def pk(golden):
    return bytes.fromhex(golden["chained"]["pk"])


@pytest.fixture(scope="module")
def base(sigs):
    """e(G1, sigma_7)^3 = e(pk, H(MessageV2(7)))^3: the module's one pairing."""
    return T.gt_base(O.g2_decompress(sigs[ROUND], check_subgroup=False))


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


# ------------------------------------------------------------------ the midstate
def test_gt_midstate_matches_hashlib(wvtest, base):
    """gtmid against hashlib over tlock_ref.encode_gt: a power of the base, the value 1, and a value with a
    coefficient whose top byte is zero (the first small power of the base that has one). The tool itself
    aborts unless the lane form's midstate is tmask_midstate's over the 576 bytes."""
    power = T.encode_gt(T.gt_pow(base, WIDE))
    acc, short = base, None
    for _ in range(4000):
        enc = T.encode_gt(acc)
        if any(enc[48 * c] == 0 for c in range(12)):
            short = enc
            break
        acc = O.f12_mul(acc, base)
    assert short is not None, "one coefficient in 21 has a zero top byte: 4,000 powers without one"
    gts = [power, T.GT_ONE, short]
    want = ["%s %s" % (hashlib.sha256(g + A.be32(0)).hexdigest(), hashlib.sha256(g + A.be32(1)).hexdigest()) for g in gts]
    assert want[1].split()[0] == A.h2(T.GT_ONE).hex()
    assert run(wvtest, "gtmid", [g.hex() for g in gts]) == want


# ------------------------------------------------------------------ the walk
def test_walk_one_wave_and_eight_match_python(wvtest):
    """awalk (wseal.h seal_walk) and tawalk (wauth.h auth_walk_team) against tlock_ref.u_of, and line for line
    against each other. 16^8 and 16^56 + 16^7 leave seven and six of the eight partial sums at infinity: the
    only place the infinity cases of the tree's complete additions are chosen on purpose (tawalk prints how
    many there were, and aborts if the partial sums stay in their slots)."""
    ks = PLAIN + SPARSE
    assert all(0 < k < R for k in ks)
    lines = ["%x" % k for k in ks]
    one = run(wvtest, "awalk", lines)
    team = run(wvtest, "tawalk", lines)
    assert [l.split()[0] for l in one] == [T.u_of(k).hex() for k in ks]
    assert [l.split()[0] for l in team] == [l.split()[0] for l in one]

    def n_inf(k):
        return sum(1 for w in range(8) if (k >> (32 * w)) & 0xFFFFFFFF == 0)
    assert [int(l.split()[1]) for l in team] == [n_inf(k) for k in ks]
    assert n_inf(16 ** 8) == 7 and n_inf(16 ** 56 + 16 ** 7) == 6 and n_inf(WIDE) == 0


# ------------------------------------------------------------------ the opening item
@pytest.fixture(scope="module")
def open_cases(base, sigs):
    """(sig, U, V, W, want sigma class, want class, want bytes) per line."""
    sig = sigs[ROUND]
    its = []
    for i, mlen in ((0, 1), (1, 33)):
        seed, msg = A.seed_of(i), A.message(i, mlen)
        its.append((msg,) + A.encrypt(base, seed, msg))
    (m0, u0, v0, w0), (m1, u1, v1, w1) = its

    def verdict(gt, u, v, w):
        msg = A.open_tail(gt, u, v, w)
        return (0, msg) if msg is not None else (AUTH, bytes(len(w)))

    def e_of(u_scalar):  # the encoded E of an item whose U is u_scalar G1, under sigma_7
        return T.encode_gt(T.gt_pow(base, u_scalar))
    k0, k1 = A.h3(A.seed_of(0), m0), A.h3(A.seed_of(1), m1)
    assert T.u_of(k0) == u0 and T.u_of(k1) == u1
    cases = []
    for (u, v, w), ku in (((u0, v0, w0), k0), ((u1, v1, w1), k1)):
        cases.append((sig, u, v, w, 0) + verdict(e_of(ku), u, v, w))
    assert [c[5:] for c in cases] == [(0, m0), (0, m1)], "the reference opens what it sealed"
    vb, wb = flip(v1, 9, 0x04), flip(w1, 32, 0x80)
    cases.append((sig, u1, vb, w1, 0) + verdict(e_of(k1), u1, vb, w1))
    cases.append((sig, u1, v1, wb, 0) + verdict(e_of(k1), u1, v1, wb))
    cases.append((sig, u0, v1, w1, 0) + verdict(e_of(k0), u0, v1, w1))  # another item's U
    # another round's signature: E is not a power of the module's base; the reference verdict needs no pairing,
    # because no E but the right one opens (checked above for E's that are powers)
    cases.append((sigs[ROUND + 1], u1, v1, w1, 0, AUTH, bytes(33)))
    cases.append((sig, INF_U, v1, w1, 0) + verdict(T.GT_ONE, INF_U, v1, w1))
    cases.append((INF_SIG, u1, v1, w1, 0) + verdict(T.GT_ONE, u1, v1, w1))
    off = T.bad_us()[O.REJ_NOT_ON_CURVE]
    cases.append((sig, off, v1, w1, 0, O.REJ_NOT_ON_CURVE, bytes(33)))
    assert [c[5] for c in cases] == [0, 0, AUTH, AUTH, AUTH, AUTH, AUTH, AUTH, O.REJ_NOT_ON_CURVE]
    return cases


def _open_lines(cases):
    return ["%s %s %s %s" % (s.hex(), u.hex(), v.hex(), w.hex()) for s, u, v, w, _, _, _ in cases]


def _open_want(cases):
    return ["%d %d %s" % (sc, c, out.hex()) for _, _, _, _, sc, c, out in cases]


def test_open_item_matches_reference(wvtest, open_cases):
    """aopen (wauth.h auth_open_item, one wave): message bytes and class against tauth_ref.open_tail."""
    assert run(wvtest, "aopen", _open_lines(open_cases)) == _open_want(open_cases)


def test_open_team_matches_reference_and_item(wvtest, open_cases):
    """taopen (auth_open_team, one host thread per wave) against the reference and line for line against aopen.
    A signature that does not decode under a U that does gives BLSV_REJ_TLOCK_SIG; under a U that does not,
    U's class comes first: compared to the one-wave form, and to the classes' precedence."""
    got = run(wvtest, "taopen", _open_lines(open_cases))
    assert got == _open_want(open_cases)
    sig, u1, v1, w1 = open_cases[1][:4]
    bad_sig = bytes([sig[0] & 0x7F]) + sig[1:]
    off = T.bad_us()[O.REJ_NOT_ON_CURVE]
    edge = ["%s %s %s %s" % (bad_sig.hex(), u.hex(), v1.hex(), w1.hex()) for u in (u1, off)]
    one = run(wvtest, "aopen", edge)
    assert run(wvtest, "taopen", edge) == one
    assert one == ["%d 9 %s" % (O.REJ_FLAG, bytes(33).hex()), "%d %d %s" % (O.REJ_FLAG, O.REJ_NOT_ON_CURVE, bytes(33).hex())]


# ------------------------------------------------------------------ the sealing item
@pytest.fixture(scope="module")
def seal_cases(base):
    out = []
    for i, mlen in ((2, 1), (3, 32), (4, 76)):
        seed, msg = A.seed_of(i), A.message(i, mlen)
        out.append((seed, msg) + A.encrypt(base, seed, msg))
    return out


def _seal_lines(pk, cases, mode="-"):
    return ["%s %d %s %s %s" % (pk.hex(), ROUND, seed.hex(), msg.hex(), mode) for seed, msg, _, _, _ in cases]


def test_seal_item_and_team_match_reference(wvtest, pk, seal_cases):
    """aseal (auth_seal_item) and taseal (auth_seal_team) against tauth_ref.encrypt, and against each other.
    (taseal also aborts if a workgroup that sealed leaves anything in the block's LDS slots.)"""
    want = ["1 %s %s %s" % (u.hex(), v.hex(), w.hex()) for _, _, u, v, w in seal_cases]
    one = run(wvtest, "aseal", _seal_lines(pk, seal_cases))
    assert one == want
    assert run(wvtest, "taseal", _seal_lines(pk, seal_cases)) == one


def test_refused_scalar_writes_zeros(wvtest, pk, seal_cases):
    """k = 0 (mod r): no SHA-256 input is known to derive it, so the tool has no honest way in through the
    derivation. Mode k0 enters behind it (auth_seal_item_k / auth_seal_team_k with the scalar zero), which
    checks the refusal's stores and ok = 0, one wave and eight -- not that a derived zero gets there."""
    lines = _seal_lines(pk, seal_cases[2:], "k0")
    want = ["0 %s %s %s" % (bytes(48).hex(), bytes(32).hex(), bytes(76).hex())]
    assert run(wvtest, "aseal", lines) == want
    assert run(wvtest, "taseal", lines) == want
