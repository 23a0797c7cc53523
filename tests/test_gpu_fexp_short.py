"""The shortened last step of the final exponentiation on the device (k_fexp.hip k_fexp_tri<0> / <4>): step 0
hands out g^3 from its x-power into a staging slot, step 4 forms t^x g^3 and compares it with conj(c^(p^4))
for the verdict, or multiplies by c^(p^4) where the value is asked for.

The values of the production stage (blsv_test_final_exp) against Python integers and the verdicts of whole
verifications against the C oracle, at the edges of the 21-items-per-wave groups of the 3-lane kernels, and
on one split pass, whose remainder runs on the side stream against the same staging slots.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 21, 22, 63, 64, 65)
CORRUPT = (20, 21, 22, 63, 64)
TOWER = (0, 2, 4, 1, 3, 5)  # w-power of the staging's Fp2 slots (soa.h st_fp12)


def _limbs(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def _words(f):
    """an oracle Fp12 (Fp2 coefficients by w-power) as the 144 raw words of blsv_test_final_exp"""
    return [w for k in TOWER for c in f[k] for w in _limbs(c)]


@pytest.fixture(scope="module")
def pool():
    """five random Fp12 values and f^(3 (p^12 - 1)/r) of each in Python integers, computed once: five is
    coprime to 3 and 21, so cycling through them puts every value on every lane role and group slot"""
    from oracle import bls12381 as O

    rng = random.Random(53)
    fs = [[(rng.randrange(O.P), rng.randrange(O.P)) for _ in range(6)] for _ in range(5)]
    return [(_words(f), _words(O.f12_pow(O.final_exponentiation(f), 3))) for f in fs]


@pytest.mark.parametrize("n", SIZES)
def test_values_equal_python_integers(engine, pool, n):
    items = [pool[(i + n) % len(pool)] for i in range(n)]
    got, ref = engine.test_final_exp([w for f, _ in items for w in f])
    want = [w for _, e in items for w in e]
    assert got == want
    assert ref == want


@pytest.fixture(scope="module")
def C():
    from oracle import c_oracle

    c_oracle.load()
    return c_oracle


@pytest.fixture()
def split(engine):
    yield engine
    engine.test_tail_split(None)


def _run(engine, golden, C, n, seg, seed, corrupt, qs):
    """verdicts of a generated history with sign-flipped signatures at `corrupt`, under every split rule of
    qs: all the same, and equal to the C oracle on the rounds in check"""
    from test_gpu_tail_split import History, _sign_flip
    from test_gpu_scale import NONE

    h = History(engine, golden, n, seg, seed=seed)
    h.put({i: _sign_flip(h.orig[i * 96:(i + 1) * 96]) for i in corrupt})
    runs = []
    for q in qs:
        engine.test_tail_split(q)
        runs.append(h.verify(engine))
    assert all(r == runs[0] for r in runs)
    ok, fb, cls = runs[0]
    assert ok == [c == 0 for c in cls]
    rejected = [i for i, c in enumerate(cls) if c]
    assert fb == (1 + rejected[0] if rejected else NONE)
    return h, cls, rejected


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_equal_c_oracle(split, golden, C, n):
    """every round of the history against the oracle; a flipped signature rejects its own round and the next"""
    corrupt = [i for i in CORRUPT if i < n]
    h, cls, rejected = _run(split, golden, C, n, 64, 59 + n, corrupt, (None,))
    assert cls == [h.oracle(C, i) for i in range(n)]
    assert rejected == sorted({j for i in corrupt for j in (i, i + 1) if j < n and (j == i or j % 64)})
    assert all(cls[i] == 7 for i in rejected)


def test_split_pass_remainder(split, golden, C):
    """65,536 + 22 items in one pass: split at 65,536 the remainder's 22 items (one full group and one item)
    run their step 0 and step 4 on the side stream, beside the main range's, on their own columns of the
    same slots. Flips at both ends of both ranges; the split, the unsplit and the device's own rule agree."""
    main, n = 65536, 65536 + 22
    corrupt = [20, main - 1, main, main + 20, n - 1]
    h, cls, rejected = _run(split, golden, C, n, 100, 61, corrupt, (main, 0, None))
    touched = sorted({j for i in corrupt for j in (i - 1, i, i + 1) if 0 <= j < n})
    assert {i: cls[i] for i in touched} == {i: h.oracle(C, i) for i in touched}
    assert rejected == [i for i in touched if cls[i]]
    assert all(cls[i] == 7 for i in corrupt)
