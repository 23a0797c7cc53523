"""The timelock item of the latency engine (drand_amd/csrc: whash.h g1_decompress, wverify.h tlock_item,
wvteam.h tlock_team) compiled for the host with wv.h's lane emulation (tools/wvtest g1dec / topen /
ttopen) and checked on the CPU against the Python oracle: the G1 decode with its reject classes, and
E = e(U, sigma)^3 in the 576-byte encoding of include/blsverify.h, one wave and eight.

One oracle pairing for the module, G = e(G1, sigma)^3 (tests/support/tlock_ref.py); every expected value
is G^r for U = r * G1. The host build checks every arithmetic contract (operand bounds, subtrahends
below their constant) as it runs, so a passing line also says the embedded G1 arithmetic keeps them."""
import os
import subprocess

import pytest

from oracle import bls12381 as O
from tests.support import tlock_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# WVTEST_TARGET=wvtest-asan runs the module on the ASan+UBSan build, as tests/test_wv_host.py does
TARGET = os.environ.get("WVTEST_TARGET", "wvtest")
BIN = os.path.join(ROOT, "tools", TARGET)

REJ_TLOCK_SIG = 9
WIDE = 0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD % O.R  # a full-width scalar
SIG_INF = b"\xc0" + bytes(95)


@pytest.fixture(scope="module")
def wvtest():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), TARGET], check=True, capture_output=True)
    return BIN


def run(binary, cmd, lines):
    r = subprocess.run([binary, cmd], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def sig(golden):
    bs = golden["chained"]["beacons"]
    return next(bytes.fromhex(b["sig_v2"]) for b in bs if b["round"] == 7)


def test_g1_decode_matches_oracle(wvtest):
    """g1dec against oracle.g1_decompress: the generator, r * G1 for small and full-width r (both sign
    bits among them), the infinity encoding, and one encoding of each reject class 2..6."""
    us = [O.g1_compress(O.G1)] + [T.u_of(r) for r in (2, 3, 5, O.R - 1, O.R - 2, WIDE, WIDE * 7 % O.R)]
    assert {u[0] & 0x20 for u in us} == {0, 0x20}, "both sign bits"
    us.append(T.u_of(0))
    bad = T.bad_us()
    us += [bad[c] for c in sorted(bad)]
    out = run(wvtest, "g1dec", [u.hex() for u in us])
    assert len(out) == len(us)
    for u, line in zip(us, out):
        f = line.split()
        cls = T.g1_class(u)
        assert int(f[0]) == cls, (u.hex(), line)
        if cls:
            assert f[1:] == ["0", "0", "0"], line
            continue
        pt = O.g1_decompress(u)
        if pt is None:
            assert f[1:] == ["1", "0", "0"], line
        else:
            assert len(f) == 4, line  # no imaginary half
            assert (f[1], int(f[2], 16), int(f[3], 16)) == ("0",) + tuple(pt), u.hex()
    assert [int(line.split()[0]) for line in out[-5:]] == [2, 3, 4, 5, 6]


@pytest.fixture(scope="module")
def cases(sig):
    """(sig96, u48, sigma's class, the item's class, the 576 bytes) per line: r in {1, 2, full width},
    the three infinity cases, one bad U of each class, one bad sigma of each class."""
    base = T.gt_base(O.g2_decompress(sig, check_subgroup=False))  # the module's one pairing
    out = [(sig, T.u_of(r), 0, 0, T.encode_gt(T.gt_pow(base, r))) for r in (1, 2, WIDE)]
    out += [(sig, T.u_of(0), 0, 0, T.GT_ONE), (SIG_INF, T.u_of(2), 0, 0, T.GT_ONE), (SIG_INF, T.u_of(0), 0, 0, T.GT_ONE)]
    out += [(sig, u, 0, c, bytes(576)) for c, u in sorted(T.bad_us().items())]
    out += [(s, T.u_of(2), c, REJ_TLOCK_SIG, bytes(576)) for c, s in sorted(T.bad_sigs(sig).items())]
    return out


def _lines(cases):
    return ["%s %s" % (s.hex(), u.hex()) for s, u, _, _, _ in cases]


def _want(cases):
    return ["%d %d %s" % (sc, c, gt.hex()) for _, _, sc, c, gt in cases]


def test_tlock_item_matches_oracle(wvtest, cases):
    """topen (wverify.h tlock_item, one wave) against tlock_ref."""
    assert run(wvtest, "topen", _lines(cases)) == _want(cases)


def test_tlock_team_matches_oracle_and_item(wvtest, cases):
    """ttopen (wvteam.h tlock_team, one host thread per wave) against tlock_ref, and line for line against
    topen; then the class of a signature alone (sig_class_team, for the rounds without items)."""
    got = run(wvtest, "ttopen", _lines(cases))
    assert got == _want(cases)
    assert got == run(wvtest, "topen", _lines(cases))
    sigs = [cases[0][0], SIG_INF] + [s for s, _, sc, _, _ in cases if sc]
    want = [0, 0] + [sc for _, _, sc, _, _ in cases if sc]
    assert run(wvtest, "ttopen", ["%s -" % s.hex() for s in sigs]) == ["%d - -" % c for c in want]
