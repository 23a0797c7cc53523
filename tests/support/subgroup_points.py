"""Points of the twist E'(Fp2) for the subgroup-check tests (tests/test_subgroup_fused_host.py,
tests/test_gpu_subgroup_fused.py), built with the Python oracle and cached per process. Every class a
test expects for them comes from the oracle's own decoder, never from this module."""
import functools
import random

from oracle import bls12381 as O

# cofactor of G2 in E'(Fp2): 13^2 and 23^2 divide it
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5


def _curve_point(rng):
    while True:
        x = (rng.randrange(O.P), rng.randrange(O.P))
        rhs = O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.B2)
        if O.f2_is_square(rhs):
            return (x, O.f2_sqrt(rhs))


@functools.lru_cache(maxsize=None)
def small_order_points(q, seed):
    """every nonzero multiple of a point of order q (13 or 23), compressed: the construction of
    tests/test_gpu_parity.py _small_order_points"""
    rng = random.Random(seed)
    while True:
        qp = O.g2_mul(_curve_point(rng), H2 * O.R // (q * q))
        if qp is None:
            continue
        base = O.g2_mul(qp, q) or qp
        assert O.g2_mul(base, q) is None
        pts, acc = [], None
        for _ in range(q - 1):
            acc = O.g2_add(acc, base)
            pts.append(O.g2_compress(acc))
        return tuple(pts)


@functools.lru_cache(maxsize=None)
def all_small_order():
    """the 12 + 22 points of order 13 and 23"""
    return small_order_points(13, 7) + small_order_points(23, 8)


@functools.lru_cache(maxsize=None)
def random_curve_points(n, seed=11):
    """n random points of E'(Fp2), compressed (outside G2 but for a chance of 1 in the cofactor)"""
    rng = random.Random(seed)
    return tuple(O.g2_compress(_curve_point(rng)) for _ in range(n))


@functools.lru_cache(maxsize=None)
def order_13r_point():
    """a point of order 13 r: the G2 generator plus a point of order 13"""
    p13 = O.g2_decompress(small_order_points(13, 7)[0], check_subgroup=False)
    pt = O.g2_add(O.G2, p13)
    assert O.g2_mul(pt, O.R) is not None and O.g2_mul(pt, 13) is not None and O.g2_mul(O.g2_mul(pt, 13), O.R) is None
    return O.g2_compress(pt)


@functools.lru_cache(maxsize=None)
def cleared_points(n, seed=12):
    """n random points of G2 (cofactor-cleared curve points), compressed"""
    rng = random.Random(seed)
    return tuple(O.g2_compress(O.g2_mul(_curve_point(rng), H2)) for _ in range(n))


def oracle_decode_class(sig):
    """the class of the oracle's decoder with its subgroup check (0 when it accepts)"""
    try:
        O.g2_decompress(sig)
    except O.DecodeError as e:
        return e.cls
    return O.REJ_OK
