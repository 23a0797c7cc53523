"""Timelock sealing on the latency path (blsv_set_tseal_lat_max, drand_amd/csrc/k_lat_tseal.hip: one
workgroup of eight waves per message) on the GPU: against the Python oracle, and byte for byte against the
batch path (mode off) for the same arguments -- U, K, ok, the zeros of a refused scalar, the error codes
with untouched outputs -- then the round trip through both opening paths, the cutover, the counters, the
caches and the setter's contract.

One oracle pairing per distinct round (tests/support/tsealr_ref.py), two in this module: the rounds 7 and 8
of the golden chain. Shapes: one workgroup per item, so n = 1, 2, 9 and 65 (more workgroups than a wave has
lanes); the scalars are window edges (1, 2, 15, the top digit alone, 63 digits of 0xF, r - 1), a full-width
value, the reductions r + 1, 2r + 5 and 2^256 - 1, and the refused 0, r and 2r, first in the batch and so in
every shape that has room for them.
"""
import ctypes

import pytest

from drand_amd import _lib
from oracle import bls12381 as O
from tests.support import tlock_ref as T
from tests.support import tseal_ref as S
from tests.support import tsealr_ref as SR

pytestmark = pytest.mark.gpu

N = 65
R = O.R
WIDE = 0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD % R
REFUSED = (0, R, 2 * R)
EDGE = [WIDE, 2 ** 256 - 1, 0, 1, 2, 15, 16 ** 63, 16 ** 63 - 1, R - 1, R + 1, 2 * R + 5, R, 2 * R]
KS = EDGE + [i + 2 for i in range(len(EDGE), N - 3)] + [WIDE * (i + 3) % R for i in (62, 63, 64)]
assert len(KS) == N and all(0 <= k < 2 ** 256 for k in KS)
OTHER_KEY = O.g1_compress(O.g1_mul(O.G1, 0x1234567))


class lat:
    """tseal_lat_max set for the duration of a block, the previous value put back."""

    def __init__(self, eng, items):
        self.eng, self.items = eng, items

    def __enter__(self):
        self.prev = self.eng.set_tseal_lat_max(self.items)

    def __exit__(self, *exc):
        self.eng.set_tseal_lat_max(self.prev)


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def pk(golden):
    return bytes.fromhex(golden["chained"]["pk"])


@pytest.fixture(scope="module")
def want(pk):
    """(round, k) -> (ok, U, K) from the oracle: one pairing per distinct round asked for, shared by the
    module, which asks for the rounds 7 and 8 alone"""
    return SR.RoundExpectations(O.g1_decompress(pk))


@pytest.fixture
def keyed(engine, pk):
    engine.set_public_key(pk)
    return engine


def triples(res):
    return [(ok, u if ok else bytes(48), g if ok else bytes(576)) for ok, u, g in zip(res.ok, res.us, res.gt)]


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("n", [1, 2, 9, 65])
def test_values(keyed, want, n):
    before = keyed.tseal_lat_stats()
    with lat(keyed, 128):
        on = keyed.tlock_seal(7, KS[:n])
    assert keyed.tseal_lat_stats() == (before[0] + 1, before[1] + n), "the call took the latency path"
    assert triples(on) == [want(7, k) for k in KS[:n]]
    assert on.ok == [k not in REFUSED for k in KS[:n]]
    with lat(keyed, 0):
        off = keyed.tlock_seal(7, KS[:n])
    assert keyed.tseal_lat_stats() == (before[0] + 1, before[1] + n)
    assert (on.ok, on.us, on.gt) == (off.ok, off.us, off.gt)


def test_rounds(keyed, want):
    """65 items over 65 distinct rounds, 0, 1 and 2^64 - 1 among them: mode on equals mode off byte for
    byte, and the items of the rounds 7 and 8 equal the oracle too."""
    rs = [0, 1, 2 ** 64 - 1, 7, 8] + [(0x9E3779B97F4A7C15 * (i + 1)) % 2 ** 64 for i in range(N - 5)]
    assert len(set(rs)) == N
    ks = KS[3:] + KS[:3]  # a plain scalar under each of the five named rounds
    before = keyed.tseal_lat_stats()
    with lat(keyed, 65):
        on = keyed.tlock_seal_rounds(rs, ks)
    assert keyed.tseal_lat_stats() == (before[0] + 1, before[1] + N)
    with lat(keyed, 0):
        off = keyed.tlock_seal_rounds(rs, ks)
    assert (on.ok, on.us, on.gt) == (off.ok, off.us, off.gt)
    assert on.ok == [k not in REFUSED for k in ks] and on.ok.count(False) == 3
    assert len(set(on.gt[:5])) == 5
    for i in (3, 4):
        assert triples(on)[i] == want(rs[i], ks[i])


def test_round_trip_through_both_openings(keyed, sigs):
    """Seals to the rounds 7 and 8 under the group key open with those rounds' signatures to the sealed K,
    on the batch path and on the opening's latency path."""
    ks = [WIDE, 2, R - 1, 16 ** 63, 2 ** 256 - 1, 15]
    rs = [7, 8, 7, 8, 8, 7]
    with lat(keyed, 8):
        one = keyed.tlock_seal(7, ks[:2])
        many = keyed.tlock_seal_rounds(rs, ks)
    assert one.ok == [True] * 2 and many.ok == [True] * 6
    assert (one.us[0], one.gt[0]) == (many.us[0], many.gt[0])
    for open_max in (0, 8):
        prev = keyed.set_tlock_lat_max(open_max)
        try:
            for r in (7, 8):
                mine = [i for i in range(6) if rs[i] == r]
                opened = keyed.tlock_open(sigs[r], [many.us[i] for i in mine])
                assert opened.ok == [True] * len(mine)
                assert opened.gt == [many.gt[i] for i in mine], (open_max, r)
            assert keyed.tlock_open(sigs[7], one.us).gt == one.gt
        finally:
            keyed.set_tlock_lat_max(prev)


# ------------------------------------------------------------------ refusal and keys
def seal_raw(eng, pk48, rnd, ks):
    """blsv_tlock_seal itself with pre-filled outputs"""
    n = len(ks)
    us = (ctypes.c_uint8 * (48 * n))(*([0xAA] * (48 * n)))
    gt = (ctypes.c_uint8 * (576 * n))(*([0xAA] * (576 * n)))
    ok = (ctypes.c_uint8 * n)(*([0xAA] * n))
    rc = eng.lib.blsv_tlock_seal(eng.handle, None if pk48 is None else _lib.buf(pk48), rnd,
                                 _lib.buf(b"".join(S.be32(k) for k in ks)), n, us, gt, ok)
    return rc, bytes(us), bytes(gt), bytes(ok)


def seal_rounds_raw(eng, pk48, rounds, ks):
    """blsv_tlock_seal_rounds itself with pre-filled outputs"""
    n = len(ks)
    us = (ctypes.c_uint8 * (48 * n))(*([0xAA] * (48 * n)))
    gt = (ctypes.c_uint8 * (576 * n))(*([0xAA] * (576 * n)))
    ok = (ctypes.c_uint8 * n)(*([0xAA] * n))
    rc = eng.lib.blsv_tlock_seal_rounds(eng.handle, None if pk48 is None else _lib.buf(pk48),
                                        (ctypes.c_uint64 * n)(*rounds), _lib.buf(b"".join(S.be32(k) for k in ks)), n,
                                        us, gt, ok)
    return rc, bytes(us), bytes(gt), bytes(ok)


def test_refused_among_good(keyed, want):
    ks = [3, 0, WIDE, R, 2 * R, 5, 2 * R + 5]
    with lat(keyed, 8):
        rc, us, gt, ok = seal_raw(keyed, None, 8, ks)
    assert rc == _lib.BLSV_OK and list(ok) == [1, 0, 1, 0, 0, 1, 1]
    for i, k in enumerate(ks):
        assert (bool(ok[i]), us[48 * i:48 * i + 48], gt[576 * i:576 * i + 576]) == want(8, k), i
    for i in (1, 3, 4):
        assert us[48 * i:48 * i + 48] == bytes(48) and gt[576 * i:576 * i + 576] == bytes(576)


def test_key_handling(keyed, pk, want):
    from drand_amd.engine import Engine
    ks, rs = [WIDE, 9], [7, 8]
    untouched = (b"\xaa" * 96, b"\xaa" * 1152, b"\xaa\xaa")
    with lat(keyed, 4):
        null = keyed.tlock_seal(7, ks)
        assert triples(null) == [want(7, k) for k in ks]
        assert triples(keyed.tlock_seal(7, ks, pk48=pk)) == triples(null), "pk48 equal to the group key"
        null_r = keyed.tlock_seal_rounds(rs, ks)
        assert triples(keyed.tlock_seal_rounds(rs, ks, pk48=pk)) == triples(null_r)
        other = keyed.tlock_seal(7, ks, pk48=OTHER_KEY)
        assert other.us == null.us and all(a != b for a, b in zip(other.gt, null.gt))
        for bad in list(T.bad_us().values()) + [b"\xc0" + bytes(47)]:
            before = keyed.tseal_lat_stats()
            rc, us, gt, ok = seal_raw(keyed, bad, 7, ks)
            assert rc == _lib.BLSV_EINVAL and (us, gt, ok) == untouched, bad.hex()
            rc, us, gt, ok = seal_rounds_raw(keyed, bad, rs, ks)
            assert rc == _lib.BLSV_EINVAL and (us, gt, ok) == untouched, bad.hex()
            assert keyed.tseal_lat_stats() == before
        with lat(keyed, 0):
            assert seal_raw(keyed, T.bad_us()[2], 7, ks)[0] == _lib.BLSV_EINVAL  # mode off: the same code
        assert triples(keyed.tlock_seal(7, ks)) == triples(null)  # the context still seals
    with Engine(0) as bare:
        bare.set_tseal_lat_max(4)
        rc, us, gt, ok = seal_raw(bare, None, 7, ks)
        assert rc == _lib.BLSV_ENOGROUP and (us, gt, ok) == untouched
        rc, us, gt, ok = seal_rounds_raw(bare, None, rs, ks)
        assert rc == _lib.BLSV_ENOGROUP and (us, gt, ok) == untouched
        assert bare.tseal_lat_stats() == (0, 0)


# ------------------------------------------------------------------ cutover and counters
def test_cutover_and_counters(pk, want):
    """L = 4: 4 items go the latency way, 5 the batch way, through both entry points. The key table counts in
    blsv_tlock_seal_rounds_stats whichever path built it; no other counter moves on a latency-path call."""
    from drand_amd.engine import Engine
    ks, rs = KS[3:8], [7, 8, 7, 8, 7]
    with Engine(0) as eng:
        eng.set_public_key(pk)
        assert eng.set_tseal_lat_max(4) == 0
        res = eng.tlock_seal(7, ks[:4])
        assert triples(res) == [want(7, k) for k in ks[:4]]
        assert eng.tseal_lat_stats() == (1, 4)
        assert eng.tlock_seal_rounds_stats() == (1, 0), "the key table is the many-rounds entry's"
        assert eng.tlock_seal_stats() == (0, 0) and eng.tlock_stats() == (0, 0)
        res = eng.tlock_seal(7, ks)
        assert triples(res) == [want(7, k) for k in ks]
        assert eng.tseal_lat_stats() == (1, 4) and eng.tlock_seal_stats() == (1, 5)
        assert eng.tlock_seal_rounds_stats() == (1, 0)
        res = eng.tlock_seal_rounds(rs[:4], ks[:4])
        assert triples(res) == [want(r, k) for r, k in zip(rs[:4], ks[:4])]
        assert eng.tseal_lat_stats() == (2, 8)
        assert eng.tlock_seal_rounds_stats() == (1, 0) and eng.tlock_seal_stats() == (1, 5)
        res = eng.tlock_seal_rounds(rs, ks)
        assert triples(res) == [want(r, k) for r, k in zip(rs, ks)]
        assert eng.tseal_lat_stats() == (2, 8)
        assert eng.tlock_seal_rounds_stats() == (1, 5), "the same key: the batch path finds the table built"
        eng.tlock_seal(8, ks[:1], pk48=OTHER_KEY)
        assert eng.tseal_lat_stats() == (3, 9) and eng.tlock_seal_rounds_stats() == (2, 5)
        assert eng.tlock_seal_stats() == (1, 5) and eng.tlock_stats() == (0, 0)
        assert eng.tlock_open_rounds_stats()[1] == 0 and eng.tlock_lat_stats() == (0, 0)


def test_caches_survive(pk, sigs, want):
    """The one-round base cache and the opening's sigma cache survive a latency-path seal."""
    from drand_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_public_key(pk)
        first = eng.tlock_seal(7, [3, WIDE])  # mode off: the base of (key, 7) built and cached
        assert triples(first) == [want(7, 3), want(7, WIDE)]
        assert eng.tlock_open(sigs[7], first.us).gt == first.gt  # sigma 7 prepared and cached
        assert eng.tlock_seal_stats() == (1, 2) and eng.tlock_stats() == (1, 2)
        with lat(eng, 4):
            assert triples(eng.tlock_seal(8, [5])) == [want(8, 5)]  # mode on, another round
            assert eng.tlock_seal_rounds([8, 7], [6, 6]).ok == [True, True]
        assert eng.tseal_lat_stats() == (2, 3)
        assert eng.tlock_seal_stats() == (1, 2) and eng.tlock_stats() == (1, 2)
        again = eng.tlock_seal(7, [3, WIDE])  # mode off again: still cached
        assert (again.us, again.gt) == (first.us, first.gt)
        assert eng.tlock_open(sigs[7], first.us).gt == first.gt
        assert eng.tlock_seal_stats() == (1, 4) and eng.tlock_stats() == (1, 4)


# ------------------------------------------------------------------ the setter's contract
def test_setter_contract(pk, want):
    from drand_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_public_key(pk)
        assert eng.set_tseal_lat_max(7) == 0, "the default is 0"
        assert eng.set_tseal_lat_max(9) == 7, "the previous value comes back"
        assert eng.set_tlock_lat_max(0) == 0, "the opening's cutover is another setting"
        prev_chunk = eng.set_chunk(16384)
        assert eng.set_tseal_lat_max(10 ** 9) == 9
        assert eng.set_tseal_lat_max(0) == 16384, "clamped to the chunk, as blsv_set_tlock_lat_max is"
        eng.set_chunk(32768)
        eng.set_tseal_lat_max(32768)
        eng.set_chunk(16384)
        assert eng.set_tseal_lat_max(0) == 16384, "a shrinking chunk clamps it too"
        eng.set_chunk(prev_chunk)
        assert triples(eng.tlock_seal(7, [3, WIDE])) == [want(7, 3), want(7, WIDE)]
        assert triples(eng.tlock_seal_rounds([8], [5])) == [want(8, 5)]
        assert eng.tseal_lat_stats() == (0, 0), "with 0 the latency path never runs"
