"""The six-column Fp4 square of the cyclotomic squaring (tri.h fp4_sqr_k6) on the device: every one of the
315 Granger-Scott squares of a final exponentiation goes through it, on all three lane roles.

The values of the production stage (blsv_test_final_exp) against Python integers and against the one-lane
reference stage, at sizes around the 21-groups-per-wave layout and its dummy lane (1, 20, 21, 22, 63, 64
items), and a 200-round chained history with one flipped signature, forced onto the batch pipeline (at this
size the engine would otherwise take the latency path, which has its own square), against the C oracle:
reject classes, accept bitmap and first_bad.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 20, 21, 22, 63, 64)
TOWER = (0, 2, 4, 1, 3, 5)  # w-power of the staging's Fp2 slots (soa.h st_fp12)


def _limbs(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def _words(f):
    """an oracle Fp12 (Fp2 coefficients by w-power) as the 144 raw words of blsv_test_final_exp"""
    return [w for k in TOWER for c in f[k] for w in _limbs(c)]


@pytest.fixture(scope="module")
def pool():
    """four random Fp12 values, one sparse one, and f^(3 (p^12 - 1)/r) of each in Python integers, computed
    once: five is coprime to 3 and 21, so cycling through them puts every value on every role and slot"""
    from oracle import bls12381 as O

    rng = random.Random(66)
    fs = [[(rng.randrange(O.P), rng.randrange(O.P)) for _ in range(6)] for _ in range(4)]
    fs.append([(rng.randrange(1, O.P), 0)] + [(0, 0)] * 4 + [(0, rng.randrange(1, O.P))])
    return [(_words(f), _words(O.f12_pow(O.final_exponentiation(f), 3))) for f in fs]


@pytest.mark.parametrize("n", SIZES)
def test_values_equal_python_integers(engine, pool, n):
    items = [pool[(i + 2 * n) % len(pool)] for i in range(n)]
    got, ref = engine.test_final_exp([w for f, _ in items for w in f])
    want = [w for _, e in items for w in e]
    assert got == want  # three lanes per item, the six-column square
    assert ref == want  # one lane per item, the tower's square


@pytest.fixture()
def batch_path(engine):
    """200 items are below the cut-over to the latency engine (1,536), which has a square of its own: force
    the batch pipeline, whose final exponentiation is k_fexp_tri, and restore the cut-over afterwards"""
    old = engine.set_lat_max(0)
    engine.profile(True)
    yield engine
    engine.profile(False)
    engine.set_lat_max(old)


def test_history_with_a_flipped_signature_equals_c_oracle(batch_path, golden):
    """200 rounds through the batch pipeline: nine full waves of 21 groups and one of 11 in every k_fexp_tri
    launch. Round 150's signature is sign-flipped (still a point of the subgroup), so the pairing check
    rejects rounds 150 and 151, whose message it chains into. The stage profile shows that the pipeline's
    final exponentiation ran once over the 200 items and the latency engine not at all."""
    from oracle import c_oracle as C
    from test_gpu_scale import NONE
    from test_gpu_tail_split import History, _sign_flip

    engine = batch_path
    C.load()
    n, bad = 200, 149
    h = History(engine, golden, n, 100, seed=67)
    h.put({bad: _sign_flip(h.orig[bad * 96:(bad + 1) * 96])})
    engine.profile_read()
    ok, first_bad, cls = h.verify(engine)
    prof = engine.profile_read()
    assert prof["final_exp"][1:] == (1, n) and prof["miller"][1:] == (1, n), prof
    assert prof["lat"][1] == 0, prof
    want = [h.oracle(C, i) for i in range(n)]
    assert cls == want
    assert [i for i, c in enumerate(want) if c] == [bad, bad + 1] and want[bad] == 7
    assert ok == [c == 0 for c in want]
    assert first_bad == bad + 1 != NONE
