"""Every field and tower form of the host build (tools/opcount ops: drand_amd/csrc/testops.h compiled
with -DBLS_HOST, KpMad in place of the LDS tables of k p) against the plain Python-integer reference
tests/support/towerref.py, on the directed operands of tests/support/opcases.py: the same items
tests/test_gpu_ops.py feeds the device. The host fuzzes of tools/opcount compare one form of the
headers with another; this is their independent reference. The coverage conditions of the operand
families (every directed value used, every quotient boundary realised, the negative branch of
fp4_sqr_k7 reached) are proven here, on a machine without a GPU. No GPU calls."""
import os
import random
import subprocess

import pytest

from oracle import bls12381 as O
from tests.support import opcases as C
from tests.support import opsuite as S
from tests.support import towerref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.P


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


@pytest.fixture(scope="module")
def host_ops(opcount_bin):
    """{name: (Fp in, Fp out, kind)} of the op list"""
    r = subprocess.run([opcount_bin, "ops", "list"], capture_output=True, text=True, check=True)
    return {f[0]: tuple(int(x) for x in f[1:]) for f in (l.split() for l in r.stdout.splitlines())}


def host_runner(opcount_bin, host_ops):
    def run(name, flat):
        nin = host_ops[name][0]
        lines = [name + " " + " ".join("%096x" % w for w in flat[i:i + nin]) for i in range(0, len(flat), nin)]
        r = subprocess.run([opcount_bin, "ops"], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [int(tok, 16) for tok in r.stdout.split()]
    return run


def one_call_runner(opcount_bin, host_ops, names):
    """all items of the given ops through ONE run of the tool (a process per batch would dominate)"""
    lines, spans = [], {}
    for name in names:
        op = S.PSEUDO.get(name, name)
        items = S.op_items(name)
        spans[name] = (len(lines), len(items))
        lines += [op + " " + " ".join("%096x" % w for w in it) for it in items]
    r = subprocess.run([opcount_bin, "ops"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    res = {}
    for name, (a, n) in spans.items():
        res[name] = [[int(t, 16) for t in l.split()] for l in out[a:a + n]]
    return res


def test_op_list_is_covered(host_ops):
    """every op of the list belongs to exactly one group and has a reference; the groups name nothing
    else"""
    grouped = [n for g in S.GROUPS.values() for n in g if n not in S.PSEUDO]
    assert sorted(grouped) == sorted(host_ops), set(grouped) ^ set(host_ops)
    assert all(n in T.REF for n in host_ops)
    assert all(host_ops[n][2] in (0, 1, 2, 3) for n in host_ops)


def test_towerref_against_oracle():
    """towerref's tower-order arithmetic against oracle/bls12381.py: the coefficient permutation, the
    product, the inverse, and the Frobenius against f12_pow(a, p) on two values"""
    rng = random.Random(3)
    for _ in range(2):
        a = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        b = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        (a0, a1, a2), (b0, b1, b2) = O.to_tower(a)
        ta = T.flat([a0, a1, a2, b0, b1, b2])
        assert ta == T.from_poly(a) and T.to_poly(ta) == a
        tb = T.from_poly(b)
        assert T.REF["fp12_mul"](ta + tb) == T.from_poly(O.f12_mul(a, b))
        inv = T.REF["fp12_inv"](ta)
        assert T.to_poly(inv) == O.f12_inv(a) and O.f12_mul(T.to_poly(inv), a) == O.F12_ONE
        assert T.to_poly(T.REF["fp12_frob"](ta)) == O.f12_pow(a, P)
        assert T.to_poly(T.REF["fp12_frob2"](T.REF["fp12_frob"](T.REF["fp12_frob"](ta)))) == \
            O.f12_frob2(O.f12_frob2(a))
        assert T.to_poly(T.REF["fp12_conj"](ta)) == O.f12_conj6(a)
        # the Fp6 and Fp4 embeddings: inverses multiply back to one, squares agree with products
        v6 = ta[:6]
        assert T.REF["fp6_mul"](T.REF["fp6_inv"](v6) + v6) == [1, 0, 0, 0, 0, 0]
        assert T.REF["fp6_sqr"](v6) == T.REF["fp6_mul"](v6 + v6)
        assert T.REF["fp4_sqr_k7"](ta[:4]) == T.REF["fp4_mul"](ta[:4] + ta[:4])
        c = T.cyclotomic(ta)  # in the cyclotomic subgroup: conj is the inverse, and c^(p^4 - p^2 + 1) = 1
        assert T.REF["fp12_mul"](c + T.REF["fp12_conj"](c)) == [1] + [0] * 11
    assert T.val(T.RP) == 1 and T.val(T.mont(5)) == 5


def test_coverage_conditions():
    """The operand families reach what they were built for, shown with Python integers alone: every
    directed value is used (asserted inside directed_cases), every (direction, k, offset, low words)
    boundary of the quotient estimate is realised in each result component of fp2_3u_pm_2x (k = 1..9)
    and kara6_c0 / c1 / c2 (every k its sum can reach), and fp4_sqr_k7's result is negative before its
    fix-up in at least 32 of the 16,384 items of its family."""
    got, want = S.quot_coverage()
    for name in want:
        for comp in (0, 1):
            assert want[name][comp] <= got[name][comp], (name, comp, sorted(want[name][comp] - got[name][comp]))
    assert len(want["fp2_3u_p_2x"][0]) == 54 and len(want["fp2_3u_m_2x"][0]) == 54
    assert [C.kara6_kmax("kara6_c0", c) for c in (0, 1)] == [13, 13]
    assert [C.kara6_kmax("kara6_c1", c) for c in (0, 1)] == [9, 9]
    assert [C.kara6_kmax("kara6_c2", c) for c in (0, 1)] == [7, 7]
    neg = S.k7_negative_count()
    print("fp4_sqr_k7 family: %d of %d negative before the fix-up" % (neg, len(C.k7_family())))
    assert len(C.k7_family()) >= 16384 and neg >= S.K7_MIN_NEGATIVE
    for name in C.CONTRACT:
        items = C.cases(name)
        used = set(w for it in items for w in it)
        for b in set(C.CONTRACT[name][0]):
            assert set(C.pool(b)) <= used, name
    for name, it in ((n, i) for n in C.CONTRACT for i in C.cases(n)):
        assert all(0 <= w < b for w, b in zip(it, C.CONTRACT[name][0])), name


@pytest.mark.parametrize("group", sorted(S.GROUPS))
def test_host_ops_match_reference(group, opcount_bin, host_ops):
    """each op of the group that the host build contains, on all of its items"""
    names = [n for n in S.GROUPS[group] if host_ops[S.PSEUDO.get(n, n)][2] == 0]
    if not names:
        assert group == "tri"  # the 3-lane forms exist on the device only (tests/test_gpu_ops.py)
        return
    res = one_call_runner(opcount_bin, host_ops, names)
    for name in names:
        op = S.PSEUDO.get(name, name)
        items = S.op_items(name)
        for it, out in zip(items, res[name]):
            err = T.check(op, it, out)
            assert err is None, "%s: %s\n  operands: %s" % (name, err, " ".join("%#x" % w for w in it))
        print("%s: %d items" % (name, len(items)))
