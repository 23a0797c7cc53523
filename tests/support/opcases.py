"""Directed operands for the raw operation hooks (drand_amd/csrc/testops.h), shared by the host run
(tests/test_ops_host.py, tools/opcount ops) and the device run (tests/test_gpu_ops.py). Everything is
seeded and generated here; there are no fixture files. Operands are raw word vectors as integers.

Per component, below the bound its operand contract states (2p for the additive forms and the tower,
any 12-word value for fp_mul / fp_sqr, 8p for the Fp2 products, 4p for the Fp2 squares):
  representatives  0, p, 1, p +- 1, 2p - 1, R mod p, R mod p + p; random v and v + p (v + k p below the
                   larger bounds) chosen independently per component
  limb patterns    2^k and 2^k - 1 for every k, p +- 2^k, 2p - 2^k; for each of the fourteen 28-bit limbs
                   of the multipliers' radix a value with that limb at 2^28 - 1 and one with it at 0, the
                   other limbs random (the top limb, bits 364.., at the largest value the bound allows)
plus the families built for one branch each: the quotient boundaries of the one-reduction linear
forms, the negative branch of fp4_sqr_k7, the structured inputs of the binary GCD, cyclotomic values."""
import random

from oracle import bls12381 as O
from . import towerref as T

P = T.P
M28 = (1 << 28) - 1
W384 = 1 << 384
D_TOP = (P >> 352) + 1  # fp_quot_top's divisor: p's top word + 1

REPS = [0, P, 1, P - 1, P + 1, 2 * P - 1, T.RP, T.RP + P]

ONE_LANE_BATCHES = (1, 63, 64, 65, 130)
TRI_BATCHES = (1, 20, 21, 22, 43, 64)

_pool_cache = {}


def pool(bound):
    """the directed values below `bound` (deterministic)"""
    if bound in _pool_cache:
        return _pool_cache[bound]
    rng = random.Random(bound % 1000003)
    out = list(REPS)
    for k in range(385):
        out += [1 << k, (1 << k) - 1]
    for k in range(382):
        out += [P + (1 << k), P - (1 << k), 2 * P - (1 << k)]
    out = [v for v in out if 0 <= v < bound]
    for j in range(14):
        s = 28 * j
        for fill in (M28, 0):
            low = rng.randrange(1 << s) if s else 0
            if j < 13:
                hi = rng.randrange(bound >> (s + 28))
                v = (hi << (s + 28)) | (fill << s) | low
            else:  # the top limb: the largest value the bound allows
                top = min(fill, (bound - 1) >> s)
                v = (top << s) | low
                if v >= bound:
                    v = (top << s) | rng.randrange(bound - (top << s))
            assert v < bound and (v >> s) & M28 == (fill if j < 13 else min(fill, (bound - 1) >> s))
            out.append(v)
    out = sorted(set(out))
    _pool_cache[bound] = out
    return out


def rnd_below(rng, bound):
    """a random residue in a random representative below the bound"""
    v = rng.randrange(P)
    kmax = (bound - 1 - v) // P
    return v + P * rng.randint(0, kmax)


def directed_cases(bounds, n, seed):
    """at least n items of len(bounds) components, more where a pool needs them: every directed value
    of each bound's pool is used at least once (asserted), half of the components directed and half
    random, so that directed values meet random partners; the items start with every representative
    in all components at once and, for two components, with every pair of representatives."""
    rng = random.Random(seed)
    nin = len(bounds)
    items = []
    for r in REPS:
        if all(r < b for b in bounds):
            items.append([r] * nin)
    if nin == 2:
        items += [[a, b] for a in REPS for b in REPS if a < bounds[0] and b < bounds[1]]
    queues = {}
    for b in set(bounds):
        q = list(pool(b))
        rng.shuffle(q)
        queues[b] = q
    pos = {b: 0 for b in queues}
    while len(items) < n or any(pos[b] < len(queues[b]) for b in queues):
        it = []
        for b in bounds:
            if rng.random() < 0.5:
                q = queues[b]
                it.append(q[pos[b] % len(q)])
                pos[b] += 1
            else:
                it.append(rnd_below(rng, b))
        items.append(it)
    for b in queues:
        assert pos[b] >= len(queues[b]), "not every directed value was used"
    return items


# ------------------------------------------------------------------ operand contracts
B2, B4, B8 = 2 * P, 4 * P, 8 * P
# name -> (bounds per component, least number of directed items)
CONTRACT = {
    "fp_mul": ([W384] * 2, 2100), "fp_mul_inl": ([W384] * 2, 2100), "fp_sqr": ([W384], 2100),
    "fp_add": ([B2] * 2, 2100), "fp_sub": ([B2] * 2, 2100), "fp_addsub_add": ([B2] * 2, 2100),
    "fp_addsub_sub": ([B2] * 2, 2100), "fp_neg": ([B2], 4000), "fp_half": ([B2], 4000),
    "fp_dbl": ([B2], 4000), "fp_mul3": ([B2], 4000), "fp_add_lazy_mul": ([B2, B2, W384], 2100),
    "fp_add_lazy2_mul": ([B2] * 5, 1040), "fp_canon": ([B2], 4000), "fp_is_zero": ([B2], 4000),
    "fp_eq": ([B2] * 2, 2100),
    "fp2_mul": ([B8] * 4, 2100), "fp2_mul_inl": ([B8] * 4, 2100), "fp2_mul_inl_kara": ([B8] * 4, 2100),
    "fp2_sqr": ([B4] * 2, 4000), "fp2_sqr_inl": ([B4] * 2, 4000), "fp2_mul_xi": ([B2] * 2, 4000),
    "fp2_neg": ([B2] * 2, 4000),
    "fp2_3u_p_2x": ([B2] * 4, 2100), "fp2_3u_m_2x": ([B2] * 4, 2100), "fp2_3u_p_2x_lds": ([B2] * 4, 2100),
    "fp2_3u_m_2x_lds": ([B2] * 4, 2100),
    "kara6_c0": ([B2] * 8, 1040), "kara6_c1": ([B2] * 8, 1040), "kara6_c2": ([B2] * 8, 1040),
    # the Fp6 products take lazily added operands (fp12_mul / fp12_sqr pass fp6_add_lazy sums)
    "fp6_mul_lin": ([B4] * 12, 1040), "fp6_mul": ([B4] * 12, 1040), "fp6_mul_lb": ([B4] * 12, 1040),
    "fp6_sqr": ([B2] * 6, 1040),
    # fp12_mul_by_014 calls it with (f.c0 + f.c1, l00, l01 + l11): a < 4p, b0 < 2p, b1 < 4p
    "fp6_mul_by_01": ([B4] * 6 + [B2] * 2 + [B4] * 2, 1040),
    "fp6_mul_by_1": ([B2] * 8, 1040), "fp6_mul_by_12": ([B2] * 10, 1040),
    "fp4_sqr_k7": ([B2] * 4, 2100), "fp4_sqr_dot": ([B2] * 4, 2100), "fp4_mul": ([B2] * 8, 1040),
    "fp12_mul": ([B2] * 24, 520), "fp12_sqr": ([B2] * 12, 520), "fp12_sqr_lin": ([B2] * 12, 520),
    "fp12_mul_by_014": ([B2] * 18, 520), "line_mul_line": ([B2] * 12, 520),
    "fp12_mul_by_line_pair_lds": ([B2] * 22, 520), "fp12_frob": ([B2] * 12, 520),
    "fp12_frob2": ([B2] * 12, 520), "fp12_conj": ([B2] * 12, 520),
    "tri_mul_lp": ([B2] * 24, 520), "tri_sqr_lp": ([B2] * 12, 520), "tri_line_pair": ([B2] * 12, 520),
    "tri_frob": ([B2] * 12, 520), "tri_frob2": ([B2] * 12, 520), "tri_conj": ([B2] * 12, 520),
}


def _seed(name):
    return sum(ord(c) * (k + 1) for k, c in enumerate(name))


_case_cache = {}


def cases(name):
    """the directed items of an op with a plain operand contract"""
    if name not in _case_cache:
        bounds, n = CONTRACT[name]
        _case_cache[name] = directed_cases(bounds, n, _seed(name))
    return _case_cache[name]


# ------------------------------------------------------------------ inversion and square root
def inv_family():
    """the structured inputs of tools/opcount invfuzz and tests/test_wv_host.py test_lane_gcd_inverse
    (2^k, 2^k - 1, p - 2^k, (p +- 1) / 2^k, p +- d, 2p - d, small values, p >> k), brought into [0, 2p),
    plus 400 random values in either representative"""
    rng = random.Random(25)
    v = [0, 1, 2, 3, P, P - 1, P - 2, P + 1, 2 * P - 1, (P + 1) // 2, (P - 1) // 2]
    for k in range(382):
        v += [1 << k, (1 << k) - 1, (P + 1) >> k, (P - 1) >> k, P >> k]
        if k < 381:
            v.append(P - (1 << k))
    for d in range(1, 64):
        v += [P - d, 2 * P - d, P + d]
    v += [rng.randrange(1, 1 << 32) for _ in range(10)]
    v = [x - 2 * P if x >= 2 * P else x for x in v]
    v += [rnd_below(rng, B2) for _ in range(400)]
    assert all(0 <= x < 2 * P for x in v)
    return [[x] for x in v]


def nonzero_items(name_seed, ncomp, n):
    """random items (either representative per component) whose value is invertible, plus the
    representatives of 1 and -1"""
    rng = random.Random(name_seed)
    items = [[T.RP] + [0] * (ncomp - 1), [T.RP + P] + [P] * (ncomp - 1), [P - T.RP] + [0] * (ncomp - 1)]
    while len(items) < n:
        items.append([rnd_below(rng, B2) for _ in range(ncomp)])
    return items


# ------------------------------------------------------------------ cyclotomic values
_cyc_cache = {}


def cyclotomic_items(n, seed=77):
    """g^((p^6 - 1)(p^2 + 1)) of random g (Python reference), every component in a representative of
    its own; the identity first (as R mod p and as R mod p + p with zeros as p)"""
    if (n, seed) in _cyc_cache:
        return _cyc_cache[(n, seed)]
    rng = random.Random(seed)
    items = [[T.RP] + [0] * 11, [T.RP + P] + [P] * 11]
    while len(items) < n:
        g = [rng.randrange(P) for _ in range(12)]
        c = T.cyclotomic(g)
        items.append([T.mont(x) + (P if rng.random() < 0.5 else 0) for x in c])
    _cyc_cache[(n, seed)] = items
    return items


# ------------------------------------------------------------------ quotient boundaries
def _solve_linear(rng, target, plus, minus, const, vals, names):
    """sets vals[x] for x in names (each in [0, 2p - 1], each appearing once in plus or minus) so that
    const + sum(plus) - sum(minus) == target; the other variables keep their values. False if the
    target is out of reach."""
    cur = const + sum(vals[x] for x in plus) - sum(vals[x] for x in minus)
    delta = target - cur
    order = list(names)
    rng.shuffle(order)
    for x in order:
        if delta == 0:
            break
        sgn = 1 if x in plus else -1
        want = vals[x] + sgn * delta
        new = min(max(want, 0), 2 * P - 1)
        delta -= sgn * (new - vals[x])
        vals[x] = new
    return delta == 0


def quot_targets(kmax):
    """(k, offset, low) -> the 385-bit sum T whose top 33 bits are k D + offset and whose low 352 bits
    are all zero (low = 0) or all ones (low = 1)"""
    out = {}
    for k in range(1, kmax + 1):
        for off in (-1, 0, 1):
            for low in (0, 1):
                out[(k, off, low)] = ((k * D_TOP + off) << 352) + (((1 << 352) - 1) if low else 0)
    return out


def sum_3u_pm_2x(u, x, sub):
    """the sum fp2_3u_pm_2x reduces: t = 3u + 2y with y = x, or 2p - x when subtracting"""
    return 3 * u + 2 * ((2 * P - x) if sub else x)


def quot_cases_3u(sub, seed=5):
    """items (u0, u1, x0, x1) of fp2_3u_pm_2x whose component sums sit on every boundary k D - 1, k D,
    k D + 1 (k = 1..9; k = 10 is out of reach since t < 10p) with the low words all zero and all ones,
    once through component 0 and once through component 1"""
    rng = random.Random(seed + int(sub))
    items = []
    for comp in (0, 1):
        for key, t in sorted(quot_targets(9).items()):
            lo = max(1, (t - 6 * P) // 2 + 1)
            hi = min(2 * P - 1, t // 2)
            y = rng.randrange(lo, hi + 1)
            while (t - 2 * y) % 3 or not (0 <= (t - 2 * y) // 3 < 2 * P) or not (1 <= y <= 2 * P - 1):
                y += 1
            u = (t - 2 * y) // 3
            x = 2 * P - y if sub else y
            assert 0 <= x < 2 * P and sum_3u_pm_2x(u, x, sub) == t
            ou, ox = rnd_below(rng, B2), rnd_below(rng, B2)
            items.append([u, ou, x, ox] if comp == 0 else [ou, u, ox, x])
    return items


# The sums T of tower.h kara6_c0 / c1 / c2 per result component, as (constant multiple of p, operands
# added, operands subtracted); operand names are indices into the item (m.c0, m.c1, t0.c0, t0.c1,
# t1.c0, t1.c1, t2.c0, t2.c1)
_M0, _M1, _T00, _T01, _T10, _T11, _T20, _T21 = range(8)
KARA6_SUMS = {
    "kara6_c0": [(6, [_M0, _T11, _T21, _T00], [_M1, _T10, _T20]),
                 (8, [_M0, _M1, _T01], [_T10, _T20, _T11, _T21])],
    "kara6_c1": [(6, [_M0, _T20], [_T00, _T10, _T21]),
                 (4, [_M1, _T20, _T21], [_T01, _T11])],
    "kara6_c2": [(4, [_M0, _T10], [_T00, _T20]),
                 (4, [_M1, _T11], [_T01, _T21])],
}


def kara6_sum(name, comp, item):
    c, plus, minus = KARA6_SUMS[name][comp]
    return c * P + sum(item[x] for x in plus) - sum(item[x] for x in minus)


def kara6_kmax(name, comp):
    """the largest k whose boundary k D + 1 the component's sum can reach: T <= c p + (2p - 1) * plus"""
    c, plus, _ = KARA6_SUMS[name][comp]
    tmax = c * P + (2 * P - 1) * len(plus)
    k = (tmax >> 352) // D_TOP
    while ((k * D_TOP + 1) << 352) + (1 << 352) - 1 > tmax:
        k -= 1
    return k


def quot_cases_kara6(name, seed=9):
    """items of kara6_c* whose sums sit on every reachable boundary, per result component"""
    rng = random.Random(seed + _seed(name))
    items = []
    for comp in (0, 1):
        c, plus, minus = KARA6_SUMS[name][comp]
        for key, t in sorted(quot_targets(kara6_kmax(name, comp)).items()):
            for _ in range(64):
                vals = [rnd_below(rng, B2) for _ in range(8)]
                if _solve_linear(rng, t, plus, minus, c * P, vals, plus + minus):
                    break
            else:
                raise AssertionError("boundary %r of %s component %d not reached" % (key, name, comp))
            assert kara6_sum(name, comp, vals) == t
            items.append(vals)
    return items


def quot_key(t):
    """(k, offset, low) of a sum if it sits on a boundary, else None"""
    top, low = t >> 352, t & ((1 << 352) - 1)
    if low == 0:
        lw = 0
    elif low == (1 << 352) - 1:
        lw = 1
    else:
        return None
    for off in (-1, 0, 1):
        if (top - off) % D_TOP == 0 and (top - off) // D_TOP >= 1:
            return ((top - off) // D_TOP, off, lw)
    return None


# ------------------------------------------------------------------ fp4_sqr_k7's negative branch
def k7_family(n=16384, seed=11):
    """(a0, a1, b0, b1) with a0 < 2^64 and a1, b0, b1 within 2^300 of 2p - 1: A = (a0 + a1)(a0 - a1)
    and -V = -2 b0 b1 are as negative as they get, so Y.a.c0 = (A + T - V + m p) / R comes out below 0
    before the conditional + p far more often than on uniform operands"""
    rng = random.Random(seed)
    near = lambda: 2 * P - 1 - rng.randrange(1 << 300)
    return [[rng.randrange(1 << 64), near(), near(), near()] for _ in range(n)]


def k7_pre_fixup(item):
    """Y.a.c0 of fp4_sqr_k7 before its conditional + p, as the exact rational (A + T - V + m p) / R"""
    a0, a1, b0, b1 = item
    s = (a0 + a1) * (a0 - a1) + (b0 + b1) * (b0 - b1) - 2 * b0 * b1
    m = (-s * pow(P, -1, T.R)) % T.R
    q, r = divmod(s + m * P, T.R)
    assert r == 0
    return q


# ------------------------------------------------------------------ batching
def batches(items, sizes):
    """consecutive batches of the given sizes, cycled until the items are used up"""
    out, k, i = [], 0, 0
    while i < len(items):
        s = sizes[k % len(sizes)]
        out.append(items[i:i + s])
        i += s
        k += 1
    return out
