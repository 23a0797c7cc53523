"""The shortened last step of the final exponentiation on the host build (tools/opcount fexp:
drand_amd/csrc/pairing.h compiled with -DBLS_HOST, the forms k_fexp.hip runs) against Python integers. No GPU.

Step 4 used to form e = t^x c^(p^2) c^-1 g^2 g and test e == 1. It now takes g^3 from step 0's x-power (|x|
starts with the bits 11), replaces c^(p^2) c^-1 by c^(p^4) (c is cyclotomic) and, for the verdict, compares
t^x g^3 with conj(c^(p^4)) instead of forming e. Checked here: the value is still f^(3 (p^12 - 1)/r), the
handed-out by-product is g g g, the p^4 Frobenius is what the identity says, and the verdict form accepts and
rejects what e == 1 does, whichever representation in [0, 2p) its operands come in.
"""
import json
import os
import random
import subprocess

import pytest

from oracle import bls12381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_GOLDEN = 4


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


def run_fexp(binp, fs):
    lines = "".join(" ".join("%x %x" % c for c in f) + "\n" for f in fs)
    r = subprocess.run([binp, "fexp"], input=lines, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout, r.stderr
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(fs)
    for o in out:
        for k in ("e", "g", "g3", "c", "frob4c"):
            v = [int(x, 16) for x in o[k]]
            o[k] = [(v[2 * j], v[2 * j + 1]) for j in range(6)]
    return out


def expected(f):
    """f^(3 (p^12 - 1)/r): the engine's convention is the cube of the oracle's reduced pairing"""
    return O.f12_pow(O.final_exponentiation(f), 3)


@pytest.fixture(scope="module")
def random_fs():
    rng = random.Random(20)
    fs = [[(rng.randrange(O.P), rng.randrange(O.P)) for _ in range(6)] for _ in range(3)]
    fs.append([(rng.randrange(1, O.P), 0)] + [(0, 0)] * 4 + [(0, rng.randrange(1, O.P))])  # sparse, zero coefficients
    return fs


@pytest.fixture(scope="module")
def golden_fs(golden):
    """the Miller values e(pk, H(m)) e(-G1, sigma) before the final exponentiation, by the oracle's Miller loop"""
    ch = golden["chained"]
    pk = O.g1_decompress(bytes.fromhex(ch["pk"]))
    neg_g1 = O.ec_neg(O.FP, O.G1)
    fs = []
    for b in ch["beacons"][:N_GOLDEN]:
        h = O.hash_to_g2(O.message(b["round"], bytes.fromhex(b["prev"])))
        s = O.g2_decompress(bytes.fromhex(b["sig"]))
        fs.append(O.f12_mul(O.miller_loop(pk, h), O.miller_loop(neg_g1, s)))
    return fs


@pytest.fixture(scope="module")
def results(opcount_bin, random_fs, golden_fs):
    return run_fexp(opcount_bin, random_fs + golden_fs)


def test_value_is_the_power_in_python_integers(results, random_fs, golden_fs):
    for f, o in zip(random_fs + golden_fs, results):
        assert O.f12_eq(o["e"], expected(f))
    for o in results[len(random_fs):]:
        assert O.f12_eq(o["e"], O.F12_ONE)


def test_by_product_is_g_cubed(results):
    for o in results:
        g = o["g"]
        assert O.f12_eq(o["g3"], O.f12_mul(O.f12_mul(g, g), g))


def test_frob4_of_a_cyclotomic_element(results):
    """c^(p^4) by constants equals the p^2 Frobenius twice and, c being cyclotomic, c^(p^2) conj(c)"""
    for o in results:
        c = o["c"]
        assert O.f12_eq(o["frob4c"], O.f12_frob2(O.f12_frob2(c)))
        assert O.f12_eq(o["frob4c"], O.f12_mul(O.f12_frob2(c), O.f12_conj6(c)))
        assert o["frob4_is_frob2_conj"] is True


def test_verdict_accepts_every_golden_pair(results, random_fs):
    """... in all four pairings of the representations [0, p) and [p, 2p) of the compared operands"""
    for o in results[len(random_fs):]:
        assert o["is_one"] is True and o["verdict"] == [True] * 4


def test_verdict_rejects(opcount_bin, results, random_fs, golden_fs):
    for o in results[:len(random_fs)]:  # random values: e != 1
        assert not O.f12_eq(o["e"], O.F12_ONE)
        assert o["is_one"] is False and o["verdict"] == [False] * 4
    # a golden value times a non-trivial pairing value (here its Miller value: e becomes e(G1, G2)^3)
    v = O.miller_loop(O.G1, O.G2)
    bad = [O.f12_mul(f, v) for f in golden_fs[:2]]
    # a golden value with one word of one coefficient flipped
    for k, (f, word) in enumerate(zip(golden_fs[:2], (0, 7))):
        g = [list(c) for c in f]
        g[(2 * k + 1) % 6][k % 2] = (g[(2 * k + 1) % 6][k % 2] ^ (0x10001 << (32 * word))) % O.P
        bad.append([tuple(c) for c in g])
    out = run_fexp(opcount_bin, bad)
    want = O.f12_pow(O.final_exponentiation(v), 3)
    assert not O.f12_eq(want, O.F12_ONE)
    for o in out[:2]:
        assert O.f12_eq(o["e"], want)
    for o in out:
        assert not O.f12_eq(o["e"], O.F12_ONE)
        assert o["is_one"] is False and o["verdict"] == [False] * 4


def test_zero_is_rejected(opcount_bin):
    """f = 0 is no Miller value; every staged value is then 0 and the two compared sides are equal. e = 0 was
    never one: the verdict form keeps rejecting it."""
    (o,) = run_fexp(opcount_bin, [[(0, 0)] * 6])
    assert o["is_one"] is False and o["verdict"] == [False] * 4


def test_op_counts(results):
    """profiles/opcount.json freezes the value form under "final_exp" (what the timelock paths pay too,
    profiles/tlock_opcount.json) and the verdict form, which a verification runs, beside it: one Fp12 product
    (54 Fp products) fewer. The value form is two Fp12 products and a cyclotomic square (2 * 54 + 18) and two
    Fp2-by-Fp scalings (c^(p^4) has four where c^(p^2) has five) below the 7,657 of the form before."""
    frozen = json.load(open(os.path.join(ROOT, "profiles", "opcount.json")))
    value, verdict = frozen["fp_mul"]["final_exp"], frozen["final_exp_verdict_fp_mul"]
    assert value == json.load(open(os.path.join(ROOT, "profiles", "tlock_opcount.json")))["fp_mul"]["final_exp"]
    for o in results:
        assert o["fp_mul"] == {"value": value, "verdict": verdict}
    assert value == verdict + 54
    assert value == 7657 - (2 * 54 + 18) - 2
