"""The split pass of the batch pipeline (verify.cpp pairing_check, hostlogic.h tail_split_main): a pass
whose single-lane Miller f pass would end in a partial wave round runs that round's items -- f pass and
final exponentiation -- on the side stream, beside the final exponentiation of the items before them.

Every verdict here is compared with the C oracle (oracle/c) on the rounds that matter and with the
unsplit engine on all of them. blsv_test_tail_split sets the round: 4,096 items instead of the device's
64 x 4 x compute units, so that a 70,003-round history splits into main = 69,632 (above the 3-lane f
pass's 64 Ki limit: the single-lane k_miller_f) and a remainder of 371.

The histories are generated on the device (tests/test_gpu_scale.py _history) in 64-round segments. With
64 | 4,096 every split falls on a segment edge, where a round's prev is a seed and not the signature
before it; the `seg` = 100 case of test 1 moves the edges (69,632 = 696 x 100 + 32) so that round
main - 1 and its successor, the remainder's first item, are chained across the split.
"""
import hashlib
import random

import pytest

from tests.support import subgroup_points as SP

pytestmark = pytest.mark.gpu

N, Q = 70003, 4096
MAIN = N - N % Q  # 69,632


@pytest.fixture(scope="module")
def C():
    from oracle import c_oracle

    c_oracle.load()
    return c_oracle


@pytest.fixture()
def split(engine):
    """the engine with its split rule, chunk and profiling restored afterwards"""
    yield engine
    engine.test_tail_split(None)
    engine.set_chunk(0)
    engine.profile(False)


def _sign_flip(sig):
    """-sigma: decodes, lies in G2, fails the pairing (the final exponentiation's REJ_PAIRING)"""
    return bytes([sig[0] ^ 0x20]) + sig[1:]


class History:
    """n generated rounds in segments of seg, with host copies for the oracle"""

    def __init__(self, engine, golden, n, seg, seed):
        from test_gpu_scale import _history

        self.n, self.seg = n, seg
        self.seeds, self.sigs, self.s0 = _history(engine, golden, n, seg, seed=seed)
        self.pk = bytes.fromhex(golden["chained"]["pk"])
        self.sd = self.seeds.cpu().numpy().tobytes()
        self.orig = self.sigs.cpu().numpy().tobytes()
        self.host = bytearray(self.orig)

    def put(self, changes):
        """the original history with {index: 96 bytes} replaced, on the device and in the host copy"""
        import torch

        self.host = bytearray(self.orig)
        for i, s in changes.items():
            assert len(s) == 96
            self.host[i * 96:(i + 1) * 96] = s
        self.sigs.copy_(torch.frombuffer(bytearray(self.host), dtype=torch.uint8).to("cuda:0"))

    def sig(self, i):
        return bytes(self.host[i * 96:(i + 1) * 96])

    def oracle(self, C, i):
        if i % self.seg == 0:
            s = i // self.seg
            prev = self.sd[s * 96: s * 96 + (self.s0 if s == 0 else 96)]
        else:
            prev = self.sig(i - 1)
        return C.verify(self.pk, hashlib.sha256(prev + (i + 1).to_bytes(8, "big")).digest(), self.sig(i))

    def verify(self, engine):
        from test_gpu_scale import _verify

        return _verify(engine, 1, self.seg, self.seeds, self.s0, self.sigs, self.n)


def _expect(h, C, touched):
    """{index: oracle class} of the touched rounds and their successors"""
    return {i: h.oracle(C, i) for i in sorted(set(touched) | {i + 1 for i in touched if i + 1 < h.n})}


def _check(h, C, got, touched):
    from test_gpu_scale import NONE

    ok, fb, cls = got
    want = _expect(h, C, touched)
    rejected = [i for i, v in enumerate(ok) if not v]
    assert rejected == [i for i, c in want.items() if c]
    assert {i: cls[i] for i in want} == want
    assert [i for i, c in enumerate(cls) if c] == rejected
    assert fb == (1 + rejected[0] if rejected else NONE)
    return want


@pytest.fixture(scope="module")
def off_curve(golden):
    mx = golden["mixed"]
    return next(bytes.fromhex(s) for s, c in zip(mx["sigs"], mx["expect_class"]) if c == 5 and len(s) == 192)


@pytest.mark.parametrize("seg", [64, 100])
def test_split_equals_unsplit_and_oracle(split, golden, C, off_curve, seg):
    """Test 1. Corrupted: the first, a middle and the last round of the main part (the last is round
    main - 1, whose successor is the remainder's first item), the first, a middle and the last round of
    the remainder (sign flips: each decodes and reaches its range's final exponentiation), and in the
    remainder a point of order 13 r (decodes, outside G2: the class the lines pass wrote must hold
    through the remainder's f pass and final exponentiation) and a point off the curve. Bitmap,
    first_bad and classes are the same with the split forced (q = 4,096), off, and at the device's own
    round (65,536 on a 256-CU device: main = 65,536 takes the 3-lane f pass, 4,467 items the side
    stream), and the forced split equals the C oracle on every touched round and its successor."""
    engine = split
    h = History(engine, golden, N, seg, seed=31)
    flips = [0, MAIN // 2 + 5, MAIN - 1, MAIN, MAIN + 185, N - 1]
    changes = {i: _sign_flip(h.orig[i * 96:(i + 1) * 96]) for i in flips}
    changes[MAIN + 100] = SP.order_13r_point()
    changes[MAIN + 200] = off_curve
    h.put(changes)
    runs = {}
    for name, q in (("split", Q), ("off", 0), ("device", None)):
        engine.test_tail_split(q)
        runs[name] = h.verify(engine)
    assert runs["split"] == runs["off"]
    assert runs["device"] == runs["off"]
    want = _check(h, C, runs["split"], list(changes))
    assert want[MAIN + 100] == 6 and want[MAIN + 200] == 5 and all(want[i] == 7 for i in flips)
    # seg = 64: round main starts a segment (its prev is a seed); seg = 100: the reject crosses the split
    assert want[MAIN] == 7 and (MAIN % seg == 0) == (seg == 64)
    if seg == 100:
        h.put({MAIN - 1: changes[MAIN - 1]})
        engine.test_tail_split(Q)
        got = h.verify(engine)
        assert _check(h, C, got, [MAIN - 1]) == {MAIN - 1: 7, MAIN: 7}


def test_two_split_passes(split, golden, C):
    """Test 2. 140,000 rounds in two passes of 70,016 and 69,984 (blsv_set_chunk), each split at 69,632:
    one corruption in the first pass's remainder, one in the second pass's main part. The second pass's
    head rewrites S, H, HQ and cls only after the first pass's side stream has joined."""
    engine = split
    n, chunk = 140_000, 70_016
    h = History(engine, golden, n, 64, seed=37)
    a, b = MAIN + 70, chunk + 1000
    assert MAIN <= a < chunk and chunk <= b < chunk + MAIN
    h.put({a: _sign_flip(h.orig[a * 96:(a + 1) * 96]), b: _sign_flip(h.orig[b * 96:(b + 1) * 96])})
    engine.set_chunk(chunk)
    engine.test_tail_split(Q)
    got = h.verify(engine)
    engine.test_tail_split(0)
    assert h.verify(engine) == got
    # the oracle also on clean rounds at both sides of the pass edge and of both splits
    want = _check(h, C, got, [a, b])
    assert want == {a: 7, a + 1: 7, b: 7, b + 1: 7}
    for i in (MAIN - 1, MAIN, chunk - 1, chunk, chunk + MAIN - 1, chunk + MAIN, n - 1):
        assert h.oracle(C, i) == 0 and got[2][i] == 0


def test_second_call_starts_clean(split, golden, C):
    """Test 3. Two calls on one context, each with its own corruption in the remainder: the second
    call's verdicts hold nothing of the first."""
    engine = split
    h = History(engine, golden, N, 64, seed=41)
    engine.test_tail_split(Q)
    first, second = MAIN + 50, MAIN + 300
    h.put({first: _sign_flip(h.orig[first * 96:(first + 1) * 96])})
    assert _check(h, C, h.verify(engine), [first]) == {first: 7, first + 1: 7}
    h.put({second: SP.random_curve_points(8)[4]})
    assert _check(h, C, h.verify(engine), [second]) == {second: 6, second + 1: 7}
    h.put({})
    ok, fb, cls = h.verify(engine)
    assert all(ok) and not any(cls)


def test_split_pass_is_one_launch_per_stage(split, golden):
    """Test 4. With profiling on, a split pass reports one miller and one final_exp launch, each over
    the whole pass (bench.py divides a stage's time and items by its launches)."""
    engine = split
    h = History(engine, golden, N, 64, seed=43)
    engine.profile(True)
    engine.profile_read()
    for q, passes, chunk in ((Q, 1, 0), (0, 1, 0), (Q, 2, 35_008)):
        engine.set_chunk(chunk)
        engine.test_tail_split(q)
        ok, fb, cls = h.verify(engine)
        assert all(ok)
        prof = engine.profile_read()
        for stage in ("miller", "final_exp", "hash", "decompress", "finish"):
            ms, launches, items = prof[stage]
            assert (launches, items) == (passes, N), (q, chunk, stage, prof[stage])
            assert ms > 0


def _limbs(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def test_final_exp_on_two_ranges(split):
    """Test 5. The final exponentiation stage on 300 random Fp12 values, whole and as the ranges
    [0, 256) and [256, 300) of the same staging (stride 300, each range with its own park area): word
    for word the same, and equal to the one-lane reference."""
    from oracle import bls12381 as O

    engine = split
    rng = random.Random(47)
    n = 300
    f = [w for _ in range(n * 12) for w in _limbs(rng.randrange(O.P))]
    engine.test_tail_split(0)
    whole, ref = engine.test_final_exp(f)
    for q in (128, 299, 21):  # [0, 256) + 44; [0, 299) + 1; [0, 294) + 6
        engine.test_tail_split(q)
        ranged, ref2 = engine.test_final_exp(f)
        assert ranged == whole, q
        assert ref2 == ref
    assert whole == ref
