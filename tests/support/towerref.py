"""Plain reference of the engine's field and tower operations: Python integers only, in the tower's
own coordinates (Fp12 = 12 Fp values in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1).

A raw word vector w (the twelve 32-bit words of a device Fp, read as one integer below 2^384) stands
for the field value w * R^-1 mod p with R = 2^392 (drand_amd/csrc/fp.h). Every expectation is stated on
those values: check(name, raw operands, raw results) asks that
  * each result is congruent to the reference mod p, and
  * each result respects the range its contract promises: below 2p, except fp_half (below 1.5p),
    fp_canon (below p) and the lazy sums, which must equal the exact integer sum; flags are 0 or 1.
No particular representative is required beyond that.

Fp2 / Fp12 arithmetic builds on oracle/bls12381.py (f2_*, f12_mul, f12_inv, f12_conj6, f12_frob2)
through the coefficient permutation tower (a0, a1, a2, b0, b1, b2) <-> polynomial [a0, b0, a1, b1,
a2, b2] that tests/test_gpu_parity.py test_pairing_golden uses."""
from oracle import bls12381 as O

P = O.P
R = 1 << 392
RINV = pow(R, -1, P)
RP = R % P
Z2 = O.F2_ZERO


def val(w):
    """field value of a raw word vector"""
    return w * RINV % P


def mont(v):
    """canonical raw word vector of a field value"""
    return v * R % P


def f2s(v):
    return [(v[2 * k], v[2 * k + 1]) for k in range(len(v) // 2)]


def flat(t):
    return [c for x in t for c in x]


def to_poly(v12):
    t = f2s(v12)
    return [t[0], t[3], t[1], t[4], t[2], t[5]]


def from_poly(a):
    return flat([a[0], a[2], a[4], a[1], a[3], a[5]])


def f6_poly(v6):
    t = f2s(v6)
    return [t[0], Z2, t[1], Z2, t[2], Z2]


def f6_from_poly(a):
    assert a[1] == Z2 and a[3] == Z2 and a[5] == Z2
    return flat([a[0], a[2], a[4]])


def f4_poly(v4):  # a + b s, s = w^3
    t = f2s(v4)
    return [t[0], Z2, Z2, t[1], Z2, Z2]


def f4_from_poly(a):
    assert a[1] == Z2 and a[2] == Z2 and a[4] == Z2 and a[5] == Z2
    return flat([a[0], a[3]])


GAMMA1 = O.f2_pow(O.XI, (P - 1) // 6)
_G1POW = [O.F2_ONE]
for _k in range(1, 6):
    _G1POW.append(O.f2_mul(_G1POW[-1], GAMMA1))


def f12_frob(a):
    """a^p on the polynomial form: c_k -> conj(c_k) gamma1^k"""
    return [O.f2_mul(O.f2_conj(a[k]), _G1POW[k]) for k in range(6)]


def cyclotomic(g12):
    """g^((p^6 - 1)(p^2 + 1)) of a tower-order value (the easy part of the final exponentiation)"""
    g = to_poly(g12)
    t = O.f12_mul(O.f12_conj6(g), O.f12_inv(g))
    return from_poly(O.f12_mul(O.f12_frob2(t), t))


def _line_poly(l6):  # sparse line (a0, a1, a4) at tower slots c0.c0, c0.c1, c1.c1
    t = f2s(l6)
    return [t[0], Z2, t[1], t[2], Z2, Z2]


def _fp_inv(a):
    return pow(a, P - 2, P)


def _kara6(which):
    def f(v):
        m, t0, t1, t2 = f2s(v)
        A, S, X = O.f2_add, O.f2_sub, lambda x: O.f2_mul(x, O.XI)
        if which == 0:
            return flat([A(X(S(S(m, t1), t2)), t0)])
        if which == 1:
            return flat([A(S(S(m, t0), t1), X(t2))])
        return flat([A(S(S(m, t0), t2), t1)])
    return f


def _f6_mul(v):
    return f6_from_poly(O.f12_mul(f6_poly(v[:6]), f6_poly(v[6:12])))


def _f6_by(slots):
    def f(v):
        b = [Z2] * 6
        for k, s in enumerate(slots):
            b[s] = (v[6 + 2 * k], v[7 + 2 * k])
        return f6_from_poly(O.f12_mul(f6_poly(v[:6]), b))
    return f


def _f4_sqr(v):
    a = f4_poly(v)
    return f4_from_poly(O.f12_mul(a, a))


def _f12_mul(v):
    return from_poly(O.f12_mul(to_poly(v[:12]), to_poly(v[12:24])))


def _f12_sqr(v):
    a = to_poly(v)
    return from_poly(O.f12_mul(a, a))


def _line_mul_line(v):
    return from_poly(O.f12_mul(_line_poly(v[:6]), _line_poly(v[6:12])))


def _line_pair(v):
    L = f2s(v[12:22])
    return from_poly(O.f12_mul(to_poly(v[:12]), [L[0], Z2, L[1], L[3], L[2], L[4]]))


def _u3(sign):
    return lambda v: [(3 * v[0] + sign * 2 * v[2]) % P, (3 * v[1] + sign * 2 * v[3]) % P]


_ONE12 = [1] + [0] * 11

# name -> reference on field values (operands in, results out)
REF = {
    "fp_mul": lambda v: [v[0] * v[1] % P],
    "fp_mul_inl": lambda v: [v[0] * v[1] % P],
    "fp_sqr": lambda v: [v[0] * v[0] % P],
    "fp_add": lambda v: [(v[0] + v[1]) % P],
    "fp_sub": lambda v: [(v[0] - v[1]) % P],
    "fp_addsub_add": lambda v: [(v[0] + v[1]) % P],
    "fp_addsub_sub": lambda v: [(v[0] - v[1]) % P],
    "fp_neg": lambda v: [-v[0] % P],
    "fp_half": lambda v: [v[0] * ((P + 1) // 2) % P],
    "fp_dbl": lambda v: [2 * v[0] % P],
    "fp_mul3": lambda v: [3 * v[0] % P],
    "fp_add_lazy_mul": lambda v: [(v[0] + v[1]) % P, (v[0] + v[1]) * v[2] % P],
    "fp_add_lazy2_mul": lambda v: [sum(v[:4]) % P, sum(v[:4]) * (v[4] + v[0]) % P],
    "fp_canon": lambda v: [v[0]],
    "fp_is_zero": lambda v: [int(v[0] == 0)],
    "fp_eq": lambda v: [int(v[0] == v[1])],
    "fp_inv_bingcd_raw": lambda v: [_fp_inv(v[0]), 1],
    "fp_inv": lambda v: [_fp_inv(v[0])],
    "fp_pow_sqrt_inv": lambda v: [pow(v[0], (P - 3) // 4, P)],
    "fp2_mul": lambda v: list(O.f2_mul((v[0], v[1]), (v[2], v[3]))),
    "fp2_sqr": lambda v: list(O.f2_mul((v[0], v[1]), (v[0], v[1]))),
    "fp2_mul_xi": lambda v: list(O.f2_mul((v[0], v[1]), O.XI)),
    "fp2_neg": lambda v: [-v[0] % P, -v[1] % P],
    "fp2_inv": lambda v: list(O.f2_inv((v[0], v[1]))) if (v[0] or v[1]) else [0, 0],
    "fp2_3u_p_2x": _u3(1),
    "fp2_3u_m_2x": _u3(-1),
    "kara6_c0": _kara6(0),
    "kara6_c1": _kara6(1),
    "kara6_c2": _kara6(2),
    "fp6_mul": _f6_mul,
    "fp6_sqr": lambda v: _f6_mul(v + v),
    "fp6_mul_by_01": _f6_by([0, 2]),
    "fp6_mul_by_1": _f6_by([2]),
    "fp6_mul_by_12": _f6_by([2, 4]),
    "fp6_inv": lambda v: f6_from_poly(O.f12_inv(f6_poly(v))),
    "fp4_sqr_k7": _f4_sqr,
    "fp4_mul": lambda v: f4_from_poly(O.f12_mul(f4_poly(v[:4]), f4_poly(v[4:8]))),
    "fp12_mul": _f12_mul,
    "fp12_sqr": _f12_sqr,
    "fp12_mul_by_014": lambda v: from_poly(O.f12_mul(to_poly(v[:12]), _line_poly(v[12:18]))),
    "line_mul_line": _line_mul_line,
    "fp12_mul_by_line_pair_lds": _line_pair,
    "fp12_cyclotomic_sqr": _f12_sqr,  # the plain Fp12 product, valid on cyclotomic inputs
    "fp12_frob": lambda v: from_poly(f12_frob(to_poly(v))),
    "fp12_frob2": lambda v: from_poly(O.f12_frob2(to_poly(v))),
    "fp12_conj": lambda v: from_poly(O.f12_conj6(to_poly(v))),
    "fp12_inv": lambda v: from_poly(O.f12_inv(to_poly(v))),
    "tri_is_one": lambda v: [int(v == _ONE12)],
}
for _alias, _of in {
    "fp2_mul_inl": "fp2_mul", "fp2_mul_inl_kara": "fp2_mul", "fp2_sqr_inl": "fp2_sqr",
    "fp2_3u_p_2x_lds": "fp2_3u_p_2x", "fp2_3u_m_2x_lds": "fp2_3u_m_2x", "fp6_mul_lin": "fp6_mul",
    "fp6_mul_lb": "fp6_mul", "fp4_sqr_dot": "fp4_sqr_k7", "fp12_sqr_lin": "fp12_sqr",
    "tri_cyclotomic_sqr": "fp12_cyclotomic_sqr", "tri_mul_lp": "fp12_mul", "tri_sqr_lp": "fp12_sqr",
    "tri_line_pair": "line_mul_line", "tri_frob": "fp12_frob", "tri_frob2": "fp12_frob2",
    "tri_conj": "fp12_conj",
}.items():
    REF[_alias] = REF[_of]

# results that are flags (exactly 0 or 1), by result index
FLAGS = {"fp_is_zero": {0}, "fp_eq": {0}, "fp_inv_bingcd_raw": {1}, "tri_is_one": {0}}
# results that are lazy sums: the exact integer sum of these raw operands
EXACT = {"fp_add_lazy_mul": {0: (0, 1)}, "fp_add_lazy2_mul": {0: (0, 1, 2, 3)}}


def bound_num_den(name):
    """(n, d): every result w of the op must satisfy d * w < n * p"""
    if name == "fp_half":
        return 3, 2
    if name == "fp_canon":
        return 1, 1
    return 2, 1


def check(name, win, wout):
    """None if the raw results wout are right for the raw operands win, else what is wrong."""
    want = REF[name]([val(w) for w in win])
    if len(want) != len(wout):
        return "%s: %d results, want %d" % (name, len(wout), len(want))
    n, d = bound_num_den(name)
    for k, (w, e) in enumerate(zip(wout, want)):
        if k in FLAGS.get(name, ()):
            if w != e:
                return "%s: flag %d is %#x, want %d" % (name, k, w, e)
            continue
        if k in EXACT.get(name, {}):
            s = sum(win[j] for j in EXACT[name][k])
            if w != s:
                return "%s: result %d is %#x, want the exact sum %#x" % (name, k, w, s)
            continue
        if val(w) != e:
            return "%s: result %d = %#x stands for %#x, want %#x" % (name, k, w, val(w), e)
        if not d * w < n * P:
            return "%s: result %d = %#x is not below %d/%d p" % (name, k, w, n, d)
    return None
