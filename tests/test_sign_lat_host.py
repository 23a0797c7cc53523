"""The signing item of the latency engine (drand_amd/csrc/wsign.h sign_item / sign_team) compiled for the
host with wv.h's lane emulation (tools/wvtest sign / tsign) and checked on the CPU against the golden
vectors and both oracles: sigma = compress([sk mod r] H(m)), one wave and eight.

The keys are chosen by their digits in base |x| (tests/support/sign_cases.py): each of the four ladders is a
64-bit left-to-right ladder on one digit, so a digit of 0, of 1, with bit 63 set and of |x| - 1 each take
another path. The host build checks every arithmetic contract (operand bounds, subtrahends below their
constant) as it runs, and tsign aborts if a workgroup leaves a partial product in its LDS slots."""
import os
import subprocess

import pytest

from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import sign_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# WVTEST_TARGET=wvtest-asan runs the module on the ASan+UBSan build, as tests/test_tseal_lat_host.py does
TARGET = os.environ.get("WVTEST_TARGET", "wvtest")
BIN = os.path.join(ROOT, "tools", TARGET)


@pytest.fixture(scope="module")
def wvtest():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), TARGET], check=True, capture_output=True)
    return BIN


def run(binary, cmd, lines):
    r = subprocess.run([binary, cmd], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().split("\n")


def line(sk, msg):
    return "%s %s" % (K.be32(sk).hex(), msg.hex() or "-")


def test_kat(wvtest, golden):
    """the vector of key/curve_test.go:10-30, one wave and eight"""
    kat = golden["kat"]
    ln = [line(int(kat["sk"], 16), bytes.fromhex(kat["msg"]))]
    assert run(wvtest, "sign", ln) == [kat["sig"]]
    assert run(wvtest, "tsign", ln) == [kat["sig"]]


def test_golden_chain(wvtest, golden):
    """two beacons of the golden chain: Message(round, prev) signs to `sig`, MessageV2(round) to `sig_v2`"""
    ch = golden["chained"]
    sk = int(ch["sk"], 16)
    lines, want = [], []
    for b in (ch["beacons"][0], ch["beacons"][5]):
        lines += [line(sk, O.message(b["round"], bytes.fromhex(b["prev"]))), line(sk, O.message_v2(b["round"]))]
        want += [b["sig"], b["sig_v2"]]
    assert run(wvtest, "tsign", lines) == want
    assert run(wvtest, "sign", lines) == want


@pytest.fixture(scope="module")
def edge_cases(golden):
    """(key, message) per line: every edge key on the 32-byte message, the KAT key on every length"""
    kat_sk = int(golden["kat"]["sk"], 16)
    return [(k, K.MSG32) for k in K.EDGE_KEYS.values()] + [(kat_sk, K.msg_of(n)) for n in K.MSG_LENS]


def test_edge_keys_and_lengths(wvtest, edge_cases):
    """tsign against oracle.c_oracle.sign for every case, against oracle.bls12381.sign for two of them, and
    line for line against sign"""
    lines = [line(k, m) for k, m in edge_cases]
    team = run(wvtest, "tsign", lines)
    assert len(team) == len(edge_cases)
    for (k, m), got in zip(edge_cases, team):
        assert got == C.sign(k, m).hex(), (hex(k), len(m))
    names = list(K.EDGE_KEYS)
    assert team[names.index("r+1")] == team[names.index("1")], "the reduction"
    assert len(set(team)) == len(team) - 1
    for i in (list(K.EDGE_KEYS).index("r-2"), len(edge_cases) - 1):  # a full-digit key; the KAT key on 300 bytes
        k, m = edge_cases[i]
        assert team[i] == O.sign(k, m).hex()
    assert run(wvtest, "sign", lines) == team


def test_zero_class(wvtest):
    """sk == 0 mod r: every digit is zero, every ladder returns the point at infinity: c0 and 95 zero bytes"""
    lines = [line(k, K.MSG32) for k in K.ZERO_KEYS.values()]
    assert run(wvtest, "tsign", lines) == [K.INF_SIG.hex()] * 3
    assert run(wvtest, "sign", lines) == [K.INF_SIG.hex()] * 3
    assert C.sign(0, K.MSG32) == K.INF_SIG
