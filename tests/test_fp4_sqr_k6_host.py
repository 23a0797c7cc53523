"""The six-column Fp4 square of the cyclotomic squaring (drand_amd/csrc/tri.h fp4_sqr_k6) on the host build
(tools/opcount.cpp compiled with -DBLS_HOST: the same function bodies the device kernels compile). No GPU.

fp4_sqr_k6 forms Y.b = 2ab from the square of the limb-wise sum a + b, so one product column fewer than
fp4_sqr_k7; its partial column sums may wrap around 2^64 and its Y.b.c0 is signed. `opcount sq6fuzz` checks it
against fp4_sqr_dot, fp4_sqr_k7 and Fp2 squares and products, every output in [0, 2p), on random operands, the
edges 0, p - 1, p, 2p - 1 in every component, operands with all limbs below the top one full, the operands
that drive Y.b.c0 to its extremes, and operands built so that Y.b.c0 is exactly -2^k before its + p; then 63
three-lane Granger-Scott squares in a row against the tower's. The tool is built with the switch BLS_FP4_SQR_K6 on (the default) and off; the final exponentiation
of the golden pairing inputs gives the same values and verdicts in both builds.
"""
import json
import os
import subprocess

import pytest

from oracle import bls12381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/llvm/bin/clang++")


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """{switch: path} of tools/opcount with BLS_FP4_SQR_K6 = 1 (the committed default, by the Makefile) and 0"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    off = str(tmp_path_factory.mktemp("opcount_k7") / "opcount")
    subprocess.run([CLANGXX, "-O2", "-std=c++17", "-DBLS_HOST", "-DBLS_FP4_SQR_K6=0", "-Wno-unknown-pragmas",
                    "-Wno-psabi", "-o", off, os.path.join(ROOT, "tools", "opcount.cpp")], check=True,
                   capture_output=True)
    return {1: os.path.join(ROOT, "tools", "opcount"), 0: off}


@pytest.mark.parametrize("switch", (1, 0))
def test_fuzz(builds, switch):
    r = subprocess.run([builds[switch], "sq6fuzz", "3000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    o = json.loads(r.stdout)
    print(o)
    assert o["k6_selected"] == switch
    assert o["cases"] >= 2 * 3000 + 256 and o["k6_mismatch"] == 0
    # the signed branch of Y.b.c0: every operand built to give exactly -2^k before the + p took it
    assert o["yb_c0_forced_cases"] >= 48 and o["yb_c0_forced_negative"] == o["yb_c0_forced_cases"]
    assert o["yb_c0_negative"] >= o["yb_c0_forced_cases"]
    assert o["cyclotomic_cases"] >= 63 and o["cyclotomic_mismatch"] == 0


def _golden_fs(golden, n=3):
    ch = golden["chained"]
    pk = O.g1_decompress(bytes.fromhex(ch["pk"]))
    neg_g1 = O.ec_neg(O.FP, O.G1)
    fs = []
    for b in ch["beacons"][:n]:
        h = O.hash_to_g2(O.message(b["round"], bytes.fromhex(b["prev"])))
        s = O.g2_decompress(bytes.fromhex(b["sig"]))
        fs.append(O.f12_mul(O.miller_loop(pk, h), O.miller_loop(neg_g1, s)))
    return fs


def test_final_exponentiation_with_the_switch_on_and_off(builds, golden):
    """final_exponentiation / final_exponentiation_is_one on golden pairing inputs and on one of them times a
    non-trivial pairing value: e = 1 and accepted, e = e(G1, G2)^3 and rejected, identically in both builds"""
    good = _golden_fs(golden)
    v = O.miller_loop(O.G1, O.G2)
    fs = good + [O.f12_mul(good[0], v)]
    lines = "".join(" ".join("%x %x" % c for c in f) + "\n" for f in fs)
    outs = {}
    for switch, binp in builds.items():
        r = subprocess.run([binp, "fexp"], input=lines, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout, r.stderr
        outs[switch] = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(outs[switch]) == len(fs)
    assert outs[1] == outs[0]
    one = ["%096x" % c for k in range(6) for c in O.F12_ONE[k]]
    for o in outs[1][:len(good)]:
        assert o["e"] == one and o["is_one"] is True and o["verdict"] == [True] * 4
    bad = outs[1][-1]
    e = [int(x, 16) for x in bad["e"]]
    assert O.f12_eq([(e[2 * j], e[2 * j + 1]) for j in range(6)], O.f12_pow(O.final_exponentiation(v), 3))
    assert bad["is_one"] is False and bad["verdict"] == [False] * 4
