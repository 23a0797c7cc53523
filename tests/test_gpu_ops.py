"""Every field and tower form as the DEVICE executes it (Engine.test_op -> blsv_test_op: the raw
operation hooks of drand_amd/csrc/testops.h in k_test.hip and k_miller.hip) against the plain
Python-integer reference tests/support/towerref.py. Operands and results are raw words, so the tests
choose the representative: the redundant range [0, 2p) is driven from outside (v and v + p, the lazy
sums below 4p and 8p the multipliers' operand contract allows, 28-bit limbs at 0 and 2^28 - 1), the
quotient estimate of the one-reduction linear forms sits on every boundary, fp4_sqr_k7's negative
branch runs, and the binary GCD must converge on every input (its exponentiation fallback would
otherwise hide a device fault). The device-only code is covered here: the LDS tables of k p, the
LDS-passed operand of fp2_mul, the Miller f pass's mf_put / mf_get forms and the 3-lane tri_*
operations with their ds_bpermute exchanges. Batches of 1, 63, 64, 65, 130 items (one lane per item)
and 1, 20, 21, 22, 43, 64 items (three lanes per item), every lane with operands of its own.

The items are those of tests/test_ops_host.py, which proves their coverage conditions without a GPU.

Run on an MI355X: python -u -m pytest -x -v -m gpu tests/test_gpu_ops.py
"""
import time

import pytest

from tests.support import opsuite as S
from tests.support import towerref as T

pytestmark = pytest.mark.gpu


def run_group(engine, group):
    ops = engine.test_ops()
    t0 = time.time()
    stats = {}
    for name in S.GROUPS[group]:
        assert S.PSEUDO.get(name, name) in ops, name  # a missing kernel is an error, never a skip
        S.run_op(engine.test_op, name, stats)
    print("%s: %s in %.2f s" % (group, ", ".join("%s %d" % kv for kv in stats.items()), time.time() - t0))


def test_op_list_matches_groups(engine):
    """the library's op list is exactly what the groups below run, with the shapes the reference has"""
    ops = engine.test_ops()
    grouped = [n for g in S.GROUPS.values() for n in g if n not in S.PSEUDO]
    assert sorted(grouped) == sorted(ops), set(grouped) ^ set(ops)
    for name, (nin, nout, lanes) in ops.items():
        assert len(S.op_items(name)[0]) == nin and len(T.REF[name](list(range(1, nin + 1)))) == nout, name
        assert lanes == (3 if name.startswith("tri_") else 1)
    with pytest.raises(KeyError):
        engine.test_op("fp_nonesuch", [0])


def test_fp_ops(engine):
    """fp_mul (called) and fp_mul_inl on any 12-word operands, fp_sqr, the add / sub / addsub / neg /
    half / dbl / mul3 chains, lazy sums (one and two levels) feeding a product, fp_canon, fp_is_zero,
    fp_eq"""
    run_group(engine, "fp")


def test_fp2_ops(engine):
    """fp2_mul (second operand through LDS, one column per lane) and both in-place bodies on operands
    below 8p, fp2_sqr / fp2_sqr_inl below 4p, fp2_mul_xi, fp2_neg"""
    run_group(engine, "fp2")


def test_linear_form_ops(engine):
    """fp2_3u_pm_2x with KpMad and with the LDS table KpLdsK<11>, kara6_c0 / c1 / c2, fp6_mul_lin and
    the f pass's fp6_mul_lb (mf_get operands) with KpLdsK<16>: fp_quot_top's float estimate, as the
    device compiler contracts and rounds it, on every boundary k D - 1, k D, k D + 1"""
    run_group(engine, "lin")


def test_fp4_fp6_ops(engine):
    """fp6_mul, fp6_sqr, fp6_mul_by_01 / _1 / _12, fp4_sqr_k7 (16,384 items of the family that makes
    its signed result negative before the conditional + p), fp4_sqr_dot, fp4_mul"""
    run_group(engine, "fp46")


def test_fp12_ops(engine):
    """fp12_mul, fp12_sqr, fp12_sqr_lin, fp12_mul_by_014, line_mul_line, the LDS line-pair product,
    fp12_cyclotomic_sqr on cyclotomic values (against the plain product), Frobenius maps, conjugate"""
    run_group(engine, "fp12")


def test_inversion_and_sqrt_ops(engine):
    """fp_inv_bingcd_raw on the structured families and 400 random values, and on every value the
    Fp2 / Fp6 / Fp12 inversions of this test hand to fp_inv: `converged` is set for all of them, so
    fp_inv's exponentiation fallback runs for none of the inputs here; fp_inv, the 4-bit-window
    a^((p-3)/4), fp2_inv, fp6_inv, fp12_inv"""
    run_group(engine, "inv")


def test_tri_ops(engine):
    """the 3-lane operations with the LDS table and the park buffer of the production launchers:
    tri_cyclotomic_sqr, tri_mul_lp, tri_sqr_lp, tri_line_pair, tri_frob, tri_frob2, tri_conj,
    tri_is_one (the identity in every representative, and off by one in each component in turn)"""
    run_group(engine, "tri")
