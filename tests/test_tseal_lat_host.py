"""The sealing item of the latency engine (drand_amd/csrc: tscalar.h, wseal.h g1_compress_store / seal_item /
seal_team) compiled for the host with wv.h's lane emulation (tools/wvtest tscalar / g1comp / tseal / ttseal)
and checked on the CPU against Python integers and the Python oracle: the scalar's reduction and digits,
the lane-form G1 compression, and (ok, U, K) with U = k G1 and K = e(k pk, H(MessageV2(round)))^3 in the
encodings of include/blsverify.h, one wave and eight.

One oracle pairing per distinct round, and two rounds (tests/support/tseal_ref.py); every expected K is a
power of its round's base. The tables the walks read are built by the batch engine's own row builder
(tseal.h), so a passing line also says the lane form reads the batch engine's entries. The host build
checks every arithmetic contract (operand bounds, subtrahends below their constant) as it runs, so it also
says the embedded G1 arithmetic of the walks keeps them."""
import os
import subprocess

import pytest

from oracle import bls12381 as O
from tests.support import tlock_ref as T
from tests.support import tseal_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# WVTEST_TARGET=wvtest-asan runs the module on the ASan+UBSan build, as tests/test_tlock_lat_host.py does
TARGET = os.environ.get("WVTEST_TARGET", "wvtest")
BIN = os.path.join(ROOT, "tools", TARGET)

R = O.R
WIDE = 0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD % R  # a full-width scalar below r
# the scalars of the issue: window edges, the top digit alone, 63 digits of 0xF, r - 1, one full-width value;
# the three reduction cases; the three refused values
PLAIN = [1, 2, 15, 16 ** 63, 16 ** 63 - 1, R - 1, WIDE]
REDUCED = [R + 1, 2 * R + 5, 2 ** 256 - 1]
REFUSED = [0, R, 2 * R]
SCALARS = PLAIN + REDUCED + REFUSED
assert all(0 <= k < 2 ** 256 for k in SCALARS) and 16 ** 63 < R
ROUND_A, ROUND_B = 7, 1000003


@pytest.fixture(scope="module")
def wvtest():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), TARGET], check=True, capture_output=True)
    return BIN


def run(binary, cmd, lines):
    r = subprocess.run([binary, cmd], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def pk(golden):
    return bytes.fromhex(golden["chained"]["pk"])


def test_scalar_reduction_and_digits(wvtest):
    """tscalar (tscalar.h tseal_scalar / tseal_digit, the form the batch kernels and the latency item share)
    against Python integers: k mod r, the refusal of 0, and the 64 four-bit digits, window 0 first."""
    out = run(wvtest, "tscalar", [S.be32(k).hex() for k in SCALARS])
    assert len(out) == len(SCALARS)
    for k, line in zip(SCALARS, out):
        ok, red, digits = line.split()
        assert int(ok) == (k % R != 0), (hex(k), line)
        assert int(red, 16) == k % R, (hex(k), line)
        assert len(digits) == 64
        assert [int(c, 16) for c in digits] == [(k % R >> (4 * w)) & 15 for w in range(64)], hex(k)
    top = out[SCALARS.index(16 ** 63)].split()[2]
    assert top == "0" * 63 + "1", "one non-zero digit, the top one"
    assert out[SCALARS.index(16 ** 63 - 1)].split()[2] == "f" * 63 + "0"


def test_g1_compress_matches_oracle(wvtest):
    """g1comp (wseal.h g1_compress_store, fed the Jacobian form so that the conversion to affine runs)
    against oracle.g1_compress: the generator, r * G1 for small and full-width r with both sign bits among
    them, and the point at infinity."""
    pts = [O.G1] + [O.g1_decompress(T.u_of(r)) for r in (2, 3, 5, R - 1, R - 2, WIDE, WIDE * 7 % R)]
    want = [O.g1_compress(p) for p in pts]
    assert {u[0] & 0x20 for u in want} == {0, 0x20}, "both sign bits"
    lines = ["%x %x" % (p[0], p[1]) for p in pts] + ["inf -"]
    want.append(O.g1_compress(None))
    assert want[-1] == b"\xc0" + bytes(47)
    assert run(wvtest, "g1comp", lines) == [u.hex() for u in want]


@pytest.fixture(scope="module")
def cases(pk):
    """(round, scalar, ok, U, K) per line: every scalar of the list under ROUND_A, the plain and one of each
    other kind under ROUND_B. Two oracle pairings."""
    pt = O.g1_decompress(pk)
    out = []
    for rnd, ks in ((ROUND_A, SCALARS), (ROUND_B, [1, WIDE, 2 * R + 5, R])):
        exp = S.Expectations(S.kbase(pt, rnd))
        out += [(rnd, k) + exp(k) for k in ks]
    return out


def _lines(pk, cases):
    return ["%s %d %s" % (pk.hex(), rnd, S.be32(k).hex()) for rnd, k, _, _, _ in cases]


def _want(cases):
    return ["%d %s %s" % (ok, u.hex(), gt.hex()) for _, _, ok, u, gt in cases]


def test_seal_item_matches_oracle(wvtest, pk, cases):
    """tseal (wseal.h seal_item, one wave) against tseal_ref: (ok, U, K) for every scalar, zeros for the
    refused ones."""
    assert sum(1 for c in cases if not c[2]) == 4
    assert run(wvtest, "tseal", _lines(pk, cases)) == _want(cases)


def test_seal_team_matches_oracle_and_item(wvtest, pk, cases):
    """ttseal (wseal.h seal_team, one host thread per wave) against tseal_ref and line for line against
    tseal. The rounds 0 and 2^64 - 1 hash without error: compared to the one-wave form only, no extra
    pairing. (ttseal also aborts if a workgroup leaves k pk in its LDS slots.)"""
    got = run(wvtest, "ttseal", _lines(pk, cases))
    assert got == _want(cases)
    edge = ["%s %d %s" % (pk.hex(), rnd, S.be32(k).hex()) for rnd, k in ((0, 2), (2 ** 64 - 1, 2), (2 ** 64 - 1, R))]
    one = run(wvtest, "tseal", _lines(pk, cases) + edge)
    assert one[:len(cases)] == got
    team = run(wvtest, "ttseal", edge)
    assert team == one[len(cases):]
    assert [line.split()[0] for line in team] == ["1", "1", "0"]
    assert team[0] != team[1], "the round reaches the hash"
    assert team[0].split()[1] == team[1].split()[1] == T.u_of(2).hex()


def test_bad_key_line(wvtest, pk):
    """the tool refuses a key that does not decode, and the point at infinity, before any walk"""
    bad = bytes([pk[0] & 0x7F]) + pk[1:]
    inf = b"\xc0" + bytes(47)
    assert run(wvtest, "tseal", ["%s 7 %s" % (k.hex(), S.be32(1).hex()) for k in (bad, inf)]) == ["-1 - -"] * 2
