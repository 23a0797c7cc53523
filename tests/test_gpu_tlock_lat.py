"""Timelock opening on the latency path (blsv_set_tlock_lat_max, drand_amd/csrc/k_lat_tlock.hip: one
workgroup of eight waves per ciphertext) on the GPU: against the Python oracle, and byte for byte against
the batch path (mode off) for the same arguments -- values, ok, classes, sig_class, untouched outputs under
a rejected sigma -- then the cutover, the counters, the sigma cache and the setter's contract.

One oracle pairing per distinct signature (tests/support/tlockr_ref.py), three in this module. Shapes: one
workgroup per item, so n = 1, 2, 9 and 65 (more workgroups than a wave has lanes, full-width scalars
among them); across rounds every kind of item and signature once.
"""
import ctypes

import pytest

from drand_amd import _lib
from oracle import bls12381 as O
from tests.support import tlock_ref as T
from tests.support import tlockr_ref as TR

pytestmark = pytest.mark.gpu

N = 65
WIDE = (0, 10, 20, 21, 22, 62, 63, 64)  # the items with full-width scalars
SIG_INF = b"\xc0" + bytes(95)


def scalar(i):
    if i in WIDE:
        return (0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD * (i + 3) + i) % O.R
    return i + 2


class lat:
    """tlock_lat_max set for the duration of a block, the previous value put back."""

    def __init__(self, eng, items):
        self.eng, self.items = eng, items

    def __enter__(self):
        self.prev = self.eng.set_tlock_lat_max(self.items)

    def __exit__(self, *exc):
        self.eng.set_tlock_lat_max(self.prev)


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def bases():
    return TR.Bases()  # one pairing per distinct signature, shared by the module


@pytest.fixture(scope="module")
def batch(sigs, bases):
    """(us, expected encodings under round 7's signature) of the 65 items, computed once."""
    rs = [scalar(i) for i in range(N)]
    return [T.u_of(r) for r in rs], TR.expected(bases, sigs[7], rs)


def as_tuple(res):
    return (res.ok, res.reject_class, res.gt)


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("n", [1, 2, 9, 65])
def test_values(engine, sigs, batch, n):
    us, want = batch
    before = engine.tlock_lat_stats()
    with lat(engine, 128):
        on = engine.tlock_open(sigs[7], us[N - n:])
    assert engine.tlock_lat_stats() == (before[0] + 1, before[1] + n), "the call took the latency path"
    assert on.ok == [True] * n and on.reject_class == [0] * n
    assert on.gt == want[N - n:]
    with lat(engine, 0):
        off = engine.tlock_open(sigs[7], us[N - n:])
    assert as_tuple(on) == as_tuple(off)


def test_rejected_us_and_infinity(engine, sigs, batch):
    """One U of each reject class and one at infinity among good ones; then sigma at infinity."""
    us, want = batch
    bad = T.bad_us()
    mixed = [us[0], bad[2], bad[3], us[3], bad[4], bad[5], T.u_of(0), bad[6], us[8]]
    with lat(engine, 16):
        on = engine.tlock_open(sigs[7], mixed)
        inf = engine.tlock_open(SIG_INF, us[:3])
    assert on.reject_class == [0, 2, 3, 0, 4, 5, 0, 6, 0]
    assert on.ok == [c == 0 for c in on.reject_class]
    assert on.gt == [want[0], None, None, want[3], None, None, T.GT_ONE, None, want[8]]
    assert inf.ok == [True] * 3 and inf.gt == [T.GT_ONE] * 3
    with lat(engine, 0):
        assert as_tuple(on) == as_tuple(engine.tlock_open(sigs[7], mixed))


# ------------------------------------------------------------------ many rounds
def open_rounds_raw(eng, sig_list, counts, flat, fill=0xAA):
    """blsv_tlock_open_rounds itself with pre-filled outputs: (rc, gt bytes, ok, classes, sig classes)"""
    n, m = len(flat), len(sig_list)
    out = (ctypes.c_uint8 * (576 * n))(*([fill] * (576 * n)))
    ok = (ctypes.c_uint8 * n)(*([fill] * n))
    cls = (ctypes.c_uint8 * n)(*([fill] * n))
    sc = (ctypes.c_uint8 * m)(*([fill] * m))
    rc = eng.lib.blsv_tlock_open_rounds(eng.handle, _lib.buf(b"".join(sig_list)), (ctypes.c_uint64 * m)(*counts), m,
                                        _lib.buf(b"".join(flat)), n, out, ok, cls, sc)
    return rc, bytes(out), list(ok), list(cls), list(sc)


def test_rounds(engine, sigs, bases):
    """Counts [2, 0, 1, 3] over four signatures: an undecodable sigma with a U that decodes (the point at
    infinity) and one that does not under it, a sigma with no items, sigma at infinity, a good sigma; the
    six U values are the point at infinity and one of each bad class. A second call mixes values that
    open with the remaining sigma classes. Mode on equals mode off byte for byte, sig_class included, and
    both equal the oracle."""
    bad = T.bad_us()
    bad_sig = T.bad_sigs(sigs[7])[5]
    sig_list = [bad_sig, sigs[8], SIG_INF, sigs[7]]
    flat = [T.u_of(0), bad[2], bad[3], bad[4], bad[5], bad[6]]
    with lat(engine, 8):
        before = engine.tlock_lat_stats()
        on = open_rounds_raw(engine, sig_list, [2, 0, 1, 3], flat)
        assert engine.tlock_lat_stats() == (before[0] + 1, before[1] + 6)
    with lat(engine, 0):
        off = open_rounds_raw(engine, sig_list, [2, 0, 1, 3], flat)
    assert on == off
    rc, gt, ok, cls, sc = on
    assert rc == _lib.BLSV_OK and sc == [5, 0, 0, 0]
    assert cls == [TR.REJ_TLOCK_SIG, 2, 3, 4, 5, 6] and ok == [0] * 6
    assert gt == bytes(6 * 576)
    # values that open, U at infinity under a good sigma, and the other classes of sigma (one without items)
    bs = T.bad_sigs(sigs[7])
    sig_list = [sigs[7], bs[2], bs[3], bs[4], bs[6], sigs[8], SIG_INF]
    flat = [bad[2], T.u_of(6), bad[3], bad[5], T.u_of(7), T.u_of(2), T.u_of(0), T.u_of(9)]
    counts = [2, 0, 1, 1, 1, 2, 1]
    with lat(engine, 8):
        on = open_rounds_raw(engine, sig_list, counts, flat)
    with lat(engine, 0):
        off = open_rounds_raw(engine, sig_list, counts, flat)
    assert on == off
    rc, gt, ok, cls, sc = on
    assert rc == _lib.BLSV_OK and sc == [0, 2, 3, 4, 6, 0, 0]
    assert cls == [2, 0, 3, 5, TR.REJ_TLOCK_SIG, 0, 0, 0] and ok == [0, 1, 0, 0, 0, 1, 1, 1]
    want = [bytes(576), TR.expected(bases, sigs[7], [6])[0], bytes(576), bytes(576), bytes(576),
            TR.expected(bases, sigs[8], [2])[0], T.GT_ONE, T.GT_ONE]
    assert [gt[576 * i:576 * i + 576] for i in range(8)] == want


# ------------------------------------------------------------------ bad sigma in blsv_tlock_open
def test_bad_sigma(engine, sigs, batch):
    from drand_amd.engine import SignatureRejected
    us, _ = batch
    with lat(engine, 4):
        for cls, s in sorted(T.bad_sigs(sigs[7]).items()):
            out = (ctypes.c_uint8 * (2 * 576))(*([0xAA] * (2 * 576)))
            ok = (ctypes.c_uint8 * 2)(0xAA, 0xAA)
            rcl = (ctypes.c_uint8 * 2)(0xAA, 0xAA)
            sc = ctypes.c_uint8(0)
            before = engine.tlock_lat_stats()
            rc = engine.lib.blsv_tlock_open(engine.handle, _lib.buf(s), _lib.buf(us[0] + us[1]), 2, out, ok, rcl,
                                            ctypes.cast(ctypes.byref(sc), _lib.u8p))
            assert engine.tlock_lat_stats()[0] == before[0] + 1, "the call took the latency path"
            assert rc == _lib.BLSV_EINVAL and sc.value == cls
            assert bytes(out) == b"\xaa" * (2 * 576) and bytes(ok) == b"\xaa\xaa" and bytes(rcl) == b"\xaa\xaa"
            with pytest.raises(SignatureRejected) as ei:
                engine.tlock_open(s, us[:2])
            assert ei.value.sig_class == cls


# ------------------------------------------------------------------ cutover and counters
def test_cutover_and_counters(engine, sigs, batch):
    us, want = batch
    with lat(engine, 4):
        l0, t0, r0 = engine.tlock_lat_stats(), engine.tlock_stats(), engine.tlock_open_rounds_stats()
        res = engine.tlock_open(sigs[7], us[:4])
        assert res.gt == want[:4]
        assert engine.tlock_lat_stats() == (l0[0] + 1, l0[1] + 4)
        assert engine.tlock_stats() == t0 and engine.tlock_open_rounds_stats() == r0
        res = engine.tlock_open(sigs[7], us[:5])
        assert res.gt == want[:5]
        assert engine.tlock_lat_stats() == (l0[0] + 1, l0[1] + 4)
        assert engine.tlock_stats()[1] == t0[1] + 5 and engine.tlock_open_rounds_stats() == r0
        # across rounds: 4 items on the latency path, 5 on the batch path
        l1, r1 = engine.tlock_lat_stats(), engine.tlock_open_rounds_stats()
        res = engine.tlock_open_rounds([sigs[7], sigs[7]], [us[:1], us[1:4]])
        assert res.gt == want[:4]
        assert engine.tlock_lat_stats() == (l1[0] + 1, l1[1] + 4) and engine.tlock_open_rounds_stats() == r1
        res = engine.tlock_open_rounds([sigs[7], sigs[7]], [us[:1], us[1:5]])
        assert res.gt == want[:5]
        assert engine.tlock_lat_stats() == (l1[0] + 1, l1[1] + 4)
        assert engine.tlock_open_rounds_stats()[1] == r1[1] + 5 and engine.tlock_stats()[1] == t0[1] + 5


# ------------------------------------------------------------------ the sigma cache survives
def test_cache_survives(sigs, batch):
    from drand_amd.engine import Engine
    us, want = batch
    with Engine(0) as eng:
        assert eng.tlock_open(sigs[7], us[:2]).gt == want[:2]  # mode off: sigma 7 prepared and cached
        assert eng.tlock_stats() == (1, 2)
        with lat(eng, 4):
            assert eng.tlock_open(sigs[8], us[:1]).ok == [True]  # mode on, another sigma
        assert eng.tlock_lat_stats() == (1, 1) and eng.tlock_stats() == (1, 2)
        assert eng.tlock_open(sigs[7], us[2:4]).gt == want[2:4]  # mode off again: still cached
        assert eng.tlock_stats() == (1, 4)


# ------------------------------------------------------------------ the setter's contract
def test_setter_contract(sigs, batch):
    from drand_amd.engine import Engine
    us, want = batch
    with Engine(0) as eng:
        assert eng.set_tlock_lat_max(7) == 0, "the default is 0"
        assert eng.set_tlock_lat_max(9) == 7, "the previous value comes back"
        prev_chunk = eng.set_chunk(16384)
        assert eng.set_tlock_lat_max(10 ** 9) == 9
        assert eng.set_tlock_lat_max(0) == 16384, "clamped to the chunk, as blsv_set_lat_max is"
        eng.set_chunk(32768)
        eng.set_tlock_lat_max(32768)
        eng.set_chunk(16384)
        assert eng.set_tlock_lat_max(0) == 16384, "a shrinking chunk clamps it too"
        eng.set_chunk(prev_chunk)
        assert eng.tlock_open(sigs[7], us[:2]).gt == want[:2]
        assert eng.tlock_open_rounds([sigs[7]], [us[:1]]).gt == want[:1]
        assert eng.tlock_lat_stats() == (0, 0), "with 0 the latency path never runs"
