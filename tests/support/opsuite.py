"""The op-level suite shared by tests/test_ops_host.py (tools/opcount ops, the host build) and
tests/test_gpu_ops.py (Engine.test_op, the device): which ops form a group, the items each op is fed
(tests/support/opcases.py) and the check of every result against tests/support/towerref.py."""
from oracle import bls12381 as O
from . import opcases as C
from . import towerref as T

P = T.P

GROUPS = {
    "fp": ["fp_mul", "fp_mul_inl", "fp_sqr", "fp_add", "fp_sub", "fp_addsub_add", "fp_addsub_sub", "fp_neg",
           "fp_half", "fp_dbl", "fp_mul3", "fp_add_lazy_mul", "fp_add_lazy2_mul", "fp_canon", "fp_is_zero", "fp_eq"],
    "fp2": ["fp2_mul", "fp2_mul_inl", "fp2_mul_inl_kara", "fp2_sqr", "fp2_sqr_inl", "fp2_mul_xi", "fp2_neg"],
    "lin": ["fp2_3u_p_2x", "fp2_3u_m_2x", "fp2_3u_p_2x_lds", "fp2_3u_m_2x_lds", "kara6_c0", "kara6_c1", "kara6_c2",
            "fp6_mul_lin", "fp6_mul_lb"],
    "fp46": ["fp6_mul", "fp6_sqr", "fp6_mul_by_01", "fp6_mul_by_1", "fp6_mul_by_12", "fp4_sqr_k7", "fp4_sqr_dot",
             "fp4_mul"],
    "fp12": ["fp12_mul", "fp12_sqr", "fp12_sqr_lin", "fp12_mul_by_014", "line_mul_line",
             "fp12_mul_by_line_pair_lds", "fp12_cyclotomic_sqr", "fp12_frob", "fp12_frob2", "fp12_conj"],
    "inv": ["fp_inv_bingcd_raw", "fp_inv", "fp_pow_sqrt_inv", "fp2_inv", "fp6_inv", "fp12_inv", "gcd_of_tower_inv"],
    "tri": ["tri_cyclotomic_sqr", "tri_mul_lp", "tri_sqr_lp", "tri_line_pair", "tri_frob", "tri_frob2", "tri_conj",
            "tri_is_one"],
}
# not an op of its own: fp_inv_bingcd_raw on the values the Fp2 / Fp6 / Fp12 inversions hand to fp_inv
PSEUDO = {"gcd_of_tower_inv": "fp_inv_bingcd_raw"}

K7_MIN_NEGATIVE = 32


def _is_one_items():
    items = [[T.RP] + [0] * 11, [T.RP + P] + [P] * 11, [T.RP] + [P] * 11]
    for k in range(12):  # off by one in a single component: every lane role must notice
        for base in (items[0], items[1]):
            it = list(base)
            it[k] += 1
            items.append(it)
        it = list(items[0])
        it[k] = (it[k] + P) if it[k] < P else it[k] - P  # the other representative: still one
        items.append(it)
    items += C.cyclotomic_items(40)[2:]
    items += [[T.RP if k == j else 0 for k in range(12)] for j in range(1, 12)]
    while len(items) < 129:
        items.append(list(items[len(items) % 3]))
    return items


def _f6_norm(v6):
    """the Fp2 value fp6_inv inverts (tower.h fp6_inv's d)"""
    a0, a1, a2 = T.f2s(v6)
    M, A, S, X = O.f2_mul, O.f2_add, O.f2_sub, lambda x: O.f2_mul(x, O.XI)
    t0 = S(M(a0, a0), X(M(a1, a2)))
    t1 = S(X(M(a2, a2)), M(a0, a1))
    t2 = S(M(a1, a1), M(a0, a2))
    return A(M(a0, t0), X(A(M(a2, t1), M(a1, t2))))


def gcd_input(name, vals):
    """the raw value fp_inv canonicalises inside fp2_inv / fp6_inv / fp12_inv of the given field values:
    the GCD starts from fp_canon of its input, so only the value counts"""
    if name == "fp2_inv":
        d = (vals[0], vals[1])
    elif name == "fp6_inv":
        d = _f6_norm(vals)
    else:
        c0, c1 = vals[:6], vals[6:]
        s1 = T.REF["fp6_mul"](c1 + c1)
        vs1 = list(O.f2_mul((s1[4], s1[5]), O.XI)) + s1[0:4]  # v (a0, a1, a2) = (xi a2, a0, a1)
        s0 = T.REF["fp6_mul"](c0 + c0)
        d = _f6_norm([(x - y) % P for x, y in zip(s0, vs1)])
    return T.mont((d[0] * d[0] + d[1] * d[1]) % P)


_items_cache = {}


def op_items(name):
    """every item the op is fed"""
    if name in _items_cache:
        return _items_cache[name]
    items = list(C.cases(name)) if name in C.CONTRACT else []
    if name.startswith("fp2_3u_"):
        items += C.quot_cases_3u("_m_" in name)
    if name.startswith("kara6_"):
        items += C.quot_cases_kara6(name)
    if name in ("fp4_sqr_k7", "fp4_sqr_dot"):
        items += C.k7_family()
    if name in ("fp_inv_bingcd_raw", "fp_inv", "fp_pow_sqrt_inv"):
        items += C.inv_family()
    if name == "fp2_inv":
        items += [[0, 0], [P, P], [0, P]] + C.nonzero_items(2, 2, 600)
    if name == "fp6_inv":
        items += C.nonzero_items(6, 6, 300)
    if name == "fp12_inv":
        items += C.nonzero_items(12, 12, 300)
    if name == "gcd_of_tower_inv":
        for op in ("fp2_inv", "fp6_inv", "fp12_inv"):
            items += [[gcd_input(op, [T.val(w) for w in it])] for it in op_items(op)]
    if name in ("fp12_cyclotomic_sqr", "tri_cyclotomic_sqr"):
        items += C.cyclotomic_items(260)
    if name == "tri_is_one":
        items += _is_one_items()
    assert items, name
    _items_cache[name] = items
    return items


def batch_sizes(name):
    return C.TRI_BATCHES if name.startswith("tri_") else C.ONE_LANE_BATCHES


def run_op(run, name, stats=None):
    """feeds the op its items through run(op name, flat operand list) -> flat result list, in batches
    of the sizes the issue lists, and checks every result; returns the number of items"""
    op = PSEUDO.get(name, name)
    items = op_items(name)
    for batch in C.batches(items, batch_sizes(name)):
        out = run(op, [w for it in batch for w in it])
        assert len(out) % len(batch) == 0 and out, (name, len(out), len(batch))
        nout = len(out) // len(batch)
        for k, it in enumerate(batch):
            err = T.check(op, it, out[k * nout:(k + 1) * nout])
            assert err is None, "%s: %s\n  operands: %s" % (name, err, " ".join("%#x" % w for w in it))
    if stats is not None:
        stats[name] = len(items)
    return len(items)


# ------------------------------------------------------------------ coverage conditions
def quot_coverage():
    """{op: boundaries realised per component} and the boundaries wanted, from the sums T of every item
    computed here with Python integers"""
    got, want = {}, {}
    for sub, names in ((False, ("fp2_3u_p_2x", "fp2_3u_p_2x_lds")), (True, ("fp2_3u_m_2x", "fp2_3u_m_2x_lds"))):
        for name in names:
            got[name] = [set(), set()]
            want[name] = [set(C.quot_targets(9)), set(C.quot_targets(9))]
            for it in op_items(name):
                for comp in (0, 1):
                    got[name][comp].add(C.quot_key(C.sum_3u_pm_2x(it[comp], it[2 + comp], sub)))
    for name in ("kara6_c0", "kara6_c1", "kara6_c2"):
        got[name] = [set(), set()]
        want[name] = [set(C.quot_targets(C.kara6_kmax(name, comp))) for comp in (0, 1)]
        for it in op_items(name):
            for comp in (0, 1):
                got[name][comp].add(C.quot_key(C.kara6_sum(name, comp, it)))
    return got, want


def k7_negative_count():
    return sum(1 for it in C.k7_family() if C.k7_pre_fixup(it) < 0)
