"""Timelock opening across many rounds on the GPU (blsv_tlock_open_rounds / _dev, drand_amd/csrc/k_tlockr.hip):
m round signatures, round j owning a run of consecutive U values. Against the Python oracle, against the
one-signature path run by run (Engine.tlock_open(sig_j, run), the contract of include/blsverify.h), and
through callers.timelock_open_rounds.

One oracle pairing per distinct signature (tests/support/tlockr_ref.py), three in this module. Shapes: a
tile is one wave (runs of 1, 63, 64, 65, 130), the 3-lane final exponentiation packs 21 items (runs of 21,
22), the pass boundary is the context chunk; both forms of the f pass are forced by dense_min, and in the
mixed form neighbouring lanes hold different signatures, so a table read from the wrong lane shows.
"""
import ctypes

import pytest

from drand_amd import _lib, callers
from tests.support import tlock_ref as T
from tests.support import tlockr_ref as TR

pytestmark = pytest.mark.gpu

ALL_UNIFORM, DEFAULT, ALL_MIXED = 1, 0, 2 ** 64 - 1
SIG_INF = b"\xc0" + bytes(95)


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    out = {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}
    assert set(range(1, 25)) <= set(out), "golden.json carries V2 signatures for rounds 1..24"
    return out


@pytest.fixture(scope="module")
def us():
    """compress((i + 1) G1), i < 746: every test's U values are a prefix (computed once)."""
    return T.consecutive_us(746)


def split(flat, counts):
    out, at = [], 0
    for k in counts:
        out.append(flat[at:at + k])
        at += k
    assert at == len(flat)
    return out


class forced:
    """dense_min set for the duration of a block, the previous value put back."""

    def __init__(self, eng, dense_min):
        self.eng, self.dense_min = eng, dense_min

    def __enter__(self):
        self.prev = self.eng.set_tlock_dense_min(self.dense_min)

    def __exit__(self, *exc):
        self.eng.set_tlock_dense_min(self.prev)


def flat_bytes(res):
    return [g if g is not None else bytes(576) for g in res.gt]


# ------------------------------------------------------------------ values
VALUE_ROUNDS, VALUE_COUNTS = (5, 6, 7, 8), (1, 65, 0, 64)


@pytest.fixture(scope="module")
def value_want(sigs, us):
    """The oracle's encodings of the 130 items: rounds 5, 6 and 8 hold items, three pairings."""
    bases = TR.Bases()
    want, at = [], 0
    for r, k in zip(VALUE_ROUNDS, VALUE_COUNTS):
        want += TR.expected(bases, sigs[r], range(at + 1, at + k + 1))
        at += k
    return want


@pytest.mark.parametrize("dense_min", [ALL_UNIFORM, DEFAULT, 2 ** 63])
def test_values(engine, sigs, us, value_want, dense_min):
    """The same bytes, the oracle's, from all-uniform tiles, the default split and all-mixed tiles."""
    engine.set_tlock_dense_min(0)
    assert engine.set_tlock_dense_min(0) == 128  # 0 restores the default, and the previous value comes back
    with forced(engine, dense_min):
        res = engine.tlock_open_rounds([sigs[r] for r in VALUE_ROUNDS], split(us[:130], VALUE_COUNTS))
    assert res.sig_class == [0, 0, 0, 0]
    assert res.ok == [True] * 130 and res.reject_class == [0] * 130
    assert res.gt == value_want


# ------------------------------------------------------------------ equality with the one-signature path
CYCLE = (1, 1, 2, 3, 21, 22, 63, 64, 65, 1, 130, 0)


@pytest.mark.parametrize("dense_min", [ALL_UNIFORM, ALL_MIXED])
def test_equals_the_one_signature_path(engine, sigs, us, dense_min):
    counts = [CYCLE[j % 12] for j in range(24)]
    assert sum(counts) == 746
    runs = split(us, counts)
    with forced(engine, dense_min):
        res = engine.tlock_open_rounds([sigs[1 + j] for j in range(24)], runs)
    assert res.sig_class == [0] * 24 and res.ok == [True] * 746
    got = split(res.gt, counts)
    for j, run in enumerate(runs):
        assert got[j] == engine.tlock_open(sigs[1 + j], run).gt, j


# ------------------------------------------------------------------ rejects
@pytest.mark.parametrize("dense_min", [ALL_UNIFORM, ALL_MIXED])
def test_rejected_us_leave_their_neighbours_alone(engine, sigs, us, dense_min):
    bad = T.bad_us()
    counts = [3, 66, 2]
    flat = list(us[:71])
    where = {1: 2, 3: 3, 40: 4, 68: 5, 70: 6}  # item -> class: inside each run, first, middle and last lanes
    for i, cls in where.items():
        flat[i] = bad[cls]
    runs = split(flat, counts)
    with forced(engine, dense_min):
        res = engine.tlock_open_rounds([sigs[5], sigs[6], sigs[7]], runs)
    assert res.sig_class == [0, 0, 0]
    assert res.reject_class == [where.get(i, 0) for i in range(71)]
    assert res.ok == [i not in where for i in range(71)]
    assert [g is None for g in res.gt] == [i in where for i in range(71)]
    got = split(res.gt, counts)
    for j, r in enumerate((5, 6, 7)):
        one = engine.tlock_open(sigs[r], runs[j])
        assert got[j] == one.gt and split(res.reject_class, counts)[j] == one.reject_class


def open_raw(eng, sig_list, counts, flat, fill=0xAA, sig_class=True):
    """blsv_tlock_open_rounds itself with pre-filled outputs: (rc, gt bytes, ok, classes, sig classes)"""
    n, m = len(flat), len(sig_list)
    out = (ctypes.c_uint8 * max(576 * n, 1))(*([fill] * max(576 * n, 1)))
    ok = (ctypes.c_uint8 * max(n, 1))(*([fill] * max(n, 1)))
    cls = (ctypes.c_uint8 * max(n, 1))(*([fill] * max(n, 1)))
    sc = (ctypes.c_uint8 * max(m, 1))(*([fill] * max(m, 1)))
    rc = eng.lib.blsv_tlock_open_rounds(eng.handle, _lib.buf(b"".join(sig_list)), (ctypes.c_uint64 * max(m, 1))(*counts),
                                        m, _lib.buf(b"".join(flat)), n, out, ok, cls, sc if sig_class else None)
    return rc, bytes(out)[:576 * n], list(ok)[:n], list(cls)[:n], list(sc)[:m]


@pytest.mark.parametrize("dense_min", [ALL_UNIFORM, ALL_MIXED])
def test_rejected_signatures(engine, sigs, us, dense_min):
    """A signature of each decode class between two good rounds: BLSV_OK, its class in sig_class, its items
    class 9 and zeros -- a rejected U under it keeps its own class -- and the other rounds as tlock_open
    gives them."""
    counts = [2, 3, 0, 2]
    flat = list(us[:7])
    flat[3] = T.bad_us()[5]
    runs = split(flat, counts)
    a, b = engine.tlock_open(sigs[5], runs[0]).gt, engine.tlock_open(sigs[6], runs[3]).gt
    for cls, bad_sig in sorted(T.bad_sigs(sigs[7]).items()):
        with forced(engine, dense_min):
            rc, gt, ok, rcl, sc = open_raw(engine, [sigs[5], bad_sig, bad_sig, sigs[6]], counts, flat)
        assert rc == _lib.BLSV_OK
        assert sc == [0, cls, cls, 0]  # the round without items is classed too
        assert rcl == [0, 0, TR.REJ_TLOCK_SIG, 5, TR.REJ_TLOCK_SIG, 0, 0] and ok == [1, 1, 0, 0, 0, 1, 1]
        assert gt == b"".join(a) + bytes(3 * 576) + b"".join(b), cls


@pytest.mark.parametrize("dense_min", [ALL_UNIFORM, ALL_MIXED])
def test_infinity(engine, sigs, us, dense_min):
    counts = [3, 2, 2]
    flat = [us[0], T.u_of(0), us[2], us[3], us[4], T.u_of(0), us[6]]
    with forced(engine, dense_min):
        res = engine.tlock_open_rounds([sigs[5], SIG_INF, sigs[6]], split(flat, counts))
    assert res.sig_class == [0, 0, 0] and res.ok == [True] * 7 and res.reject_class == [0] * 7
    assert [g == T.GT_ONE for g in res.gt] == [False, True, False, True, True, True, False]
    assert res.gt[:3] == engine.tlock_open(sigs[5], flat[:3]).gt and res.gt[5:] == engine.tlock_open(sigs[6], flat[5:]).gt


# ------------------------------------------------------------------ pass boundary
def test_pass_boundary(sigs):
    """n = chunk + 65 with the chunk capped at 16,384, three signatures, the middle run straddling the
    boundary: the same bytes as one pass, every run what tlock_open gives for its round, and the straddling
    run prepared in both passes."""
    from drand_amd.engine import Engine
    n = 16384 + 65
    counts = [100, 16384 - 100 + 30, 35]
    flat = T.consecutive_us(n)
    runs = split(flat, counts)
    three = [sigs[5], sigs[6], sigs[7]]
    with Engine(0) as eng:
        whole = eng.tlock_open_rounds(three, runs)
        assert eng.tlock_open_rounds_stats() == (3, n)
        prev = eng.set_chunk(16384)
        try:
            capped = eng.tlock_open_rounds(three, runs)
            assert eng.tlock_open_rounds_stats() == (3 + 4, 2 * n)
            assert whole.ok == [True] * n and capped.ok == whole.ok and capped.sig_class == whole.sig_class == [0, 0, 0]
            assert capped.gt == whole.gt
            got = split(whole.gt, counts)
            for j in range(3):
                assert got[j] == eng.tlock_open(three[j], runs[j]).gt, j
        finally:
            eng.set_chunk(prev)


# ------------------------------------------------------------------ device-pointer form
def test_dev_form_equals_host_form(engine, sigs, us):
    import torch
    counts = [2, 0, 66, 3]
    n, m = 71, 4
    flat = list(us[:n])
    flat[5] = T.bad_us()[5]
    four = [sigs[5], T.bad_sigs(sigs[7])[4], sigs[6], T.bad_sigs(sigs[7])[2]]
    dev = torch.device("cuda", 0)
    packed = b"".join(flat)
    d_us = torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(dev)
    d_out = torch.full((n * 576,), 0xAA, dtype=torch.uint8, device=dev)
    d_cls = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    d_sc = torch.full((m,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)  # the fills run on torch's stream, the engine on its own
    engine.tlock_open_rounds_dev(four, counts, d_us.data_ptr(), n, d_out.data_ptr(), d_cls.data_ptr(), d_sc.data_ptr())
    engine.synchronize()
    torch.cuda.synchronize(dev)
    host = engine.tlock_open_rounds(four, split(flat, counts))
    ob = bytes(d_out.cpu().numpy())
    assert [ob[576 * i:576 * i + 576] for i in range(n)] == flat_bytes(host)
    assert list(d_cls.cpu().numpy()) == host.reject_class and list(d_sc.cpu().numpy()) == host.sig_class == [0, 4, 0, 2]
    assert host.reject_class == [0, 0] + [0, 0, 0, 5] + [0] * 62 + [TR.REJ_TLOCK_SIG] * 3
    assert bytes(d_us.cpu().numpy()) == packed  # the caller's buffer is only read
    # the optional outputs may be absent
    d_out2 = torch.full((n * 576,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    engine.tlock_open_rounds_dev(four, counts, d_us.data_ptr(), n, d_out2.data_ptr())
    engine.synchronize()
    assert bytes(d_out2.cpu().numpy()) == ob


# ------------------------------------------------------------------ caches and counters
def test_caches_and_counters(sigs, us, golden):
    """Nothing is cached and no other counter moves: an opening under one sigma before and after the call
    prepares once; tlock_open_rounds_stats counts each decodable sigma with items once per pass, and the U
    values."""
    from drand_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_public_key(bytes.fromhex(golden["chained"]["pk"]))
        assert eng.tlock_open_rounds_stats() == (0, 0)
        before = eng.tlock_open(sigs[5], us[:2]).gt
        sealed = eng.tlock_seal(9, [3, 5])
        sealed_r = eng.tlock_seal_rounds([9, 10], [3, 5])
        stats = (eng.tlock_stats(), eng.tlock_seal_stats(), eng.tlock_seal_rounds_stats())
        assert stats == ((1, 2), (1, 2), (1, 2))
        counts = [2, 0, 1, 3, 1]
        five = [sigs[5], sigs[6], T.bad_sigs(sigs[7])[5], sigs[8], SIG_INF]
        res = eng.tlock_open_rounds(five, split(us[:7], counts))
        assert res.sig_class == [0, 0, 5, 0, 0] and res.gt[:2] == before
        assert eng.tlock_open_rounds_stats() == (3, 7)  # sigs 5 and 8 and the point at infinity; not 6 (no items)
        assert (eng.tlock_stats(), eng.tlock_seal_stats(), eng.tlock_seal_rounds_stats()) == stats
        assert eng.tlock_open(sigs[5], us[:2]).gt == before
        assert eng.tlock_stats() == (1, 4)  # the cached sigma survived the call
        again, again_r = eng.tlock_seal(9, [3, 5]), eng.tlock_seal_rounds([9, 10], [3, 5])
        assert (again.us, again.gt, again_r.gt) == (sealed.us, sealed.gt, sealed_r.gt)
        assert eng.tlock_seal_stats() == (1, 4) and eng.tlock_seal_rounds_stats() == (1, 4)
        eng.tlock_open_rounds(five[:1], [us[:1]])
        assert eng.tlock_open_rounds_stats() == (4, 8)  # the same sigma again is prepared again


# ------------------------------------------------------------------ argument errors
def test_argument_errors(engine, sigs, us):
    import torch
    two = [sigs[5], sigs[6]]
    flat = list(us[:4])
    for counts in ([2, 1], [2, 3], [2 ** 64 - 1, 5]):  # the sum is not n, or wraps to it
        rc, gt, ok, rcl, sc = open_raw(engine, two, counts, flat)
        assert rc == _lib.BLSV_EINVAL
        assert (gt, ok, rcl, sc) == (b"\xaa" * (4 * 576), [0xAA] * 4, [0xAA] * 4, [0xAA] * 2)
    lib, h = engine.lib, engine.handle
    sb, cn, ub = _lib.buf(b"".join(two)), (ctypes.c_uint64 * 2)(2, 2), _lib.buf(b"".join(flat))
    out = (ctypes.c_uint8 * (4 * 576))(*([0xAA] * (4 * 576)))
    ok = (ctypes.c_uint8 * 4)(*([0xAA] * 4))
    for args in ((None, cn, 2, ub, 4, out, ok), (sb, None, 2, ub, 4, out, ok), (sb, cn, 2, None, 4, out, ok),
                 (sb, cn, 2, ub, 4, None, ok), (sb, cn, 2, ub, 4, out, None)):
        assert lib.blsv_tlock_open_rounds(h, *args, None, None) == _lib.BLSV_EINVAL
    assert bytes(out) == b"\xaa" * (4 * 576) and bytes(ok) == b"\xaa" * 4
    assert lib.blsv_tlock_open_rounds(None, sb, cn, 2, ub, 4, out, ok, None, None) == _lib.BLSV_EINVAL
    dev = torch.device("cuda", 0)
    d_us = torch.frombuffer(bytearray(b"".join(flat)), dtype=torch.uint8).to(dev)
    d_out = torch.full((4 * 576 + 4,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    p_us, p_out = d_us.data_ptr(), d_out.data_ptr()
    assert p_out % 4 == 0
    for args in ((sb, cn, 2, p_us, 4, p_out + 1), (sb, cn, 2, None, 4, p_out), (sb, cn, 2, p_us, 4, None),
                 (None, cn, 2, p_us, 4, p_out), (sb, (ctypes.c_uint64 * 2)(2, 1), 2, p_us, 4, p_out)):
        assert lib.blsv_tlock_open_rounds_dev(h, *args, None, None, None) == _lib.BLSV_EINVAL
    engine.synchronize()
    assert bytes(d_out.cpu().numpy()) == b"\xaa" * (4 * 576 + 4)
    # no rounds and no items is a call that does nothing
    assert lib.blsv_tlock_open_rounds(h, None, None, 0, None, 0, None, None, None, None) == _lib.BLSV_OK


# ------------------------------------------------------------------ end to end
def test_timelock_open_rounds_end_to_end(engine, golden, sigs):
    """callers.timelock_seal_rounds over four messages and three rounds, then callers.timelock_open_rounds:
    with verify=True the messages come back; under the next round's signatures it raises, and with
    verify=False it returns other bytes of the same lengths."""
    engine.set_public_key(bytes.fromhex(golden["chained"]["pk"]))
    msgs = [b"", b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100))]
    sealed_to = [3, 9, 3, 17]
    cts = callers.timelock_seal_rounds(engine, list(zip(sealed_to, msgs)), callers.kdf_sha256_ctr)
    order = sorted(set(sealed_to))
    mine = {r: [i for i in range(4) if sealed_to[i] == r] for r in order}
    rounds = [(r, sigs[r], [cts[i] for i in mine[r]] + ([(T.bad_us()[6], b"locked to nothing")] if r == 9 else []))
              for r in order]
    got = callers.timelock_open_rounds(engine, rounds, callers.kdf_sha256_ctr)
    assert got == [[msgs[0], msgs[2]], [msgs[1], None], [msgs[3]]]
    nxt = [(r, sigs[r + 1], c) for r, _, c in rounds]
    with pytest.raises(callers.VerifyError) as ei:
        callers.timelock_open_rounds(engine, nxt, callers.kdf_sha256_ctr)
    assert ei.value.round == 3
    wrong = callers.timelock_open_rounds(engine, nxt, callers.kdf_sha256_ctr, verify=False)
    assert [[None if w is None else len(w) for w in ws] for ws in wrong] == [[0, 32], [1, None], [100]]
    assert wrong[0][1] != msgs[2] and wrong[2][0] != msgs[3]
