"""The authenticated timelock on the latency path (blsv_set_tauth_lat_max; drand_amd/csrc/k_lat_tauth_open.hip,
k_lat_tauth_seal.hip, tauth_lat.cpp): one workgroup per item, one launch per call.

Expected bytes never come from the code under test: tests/support/tauth_ref.py (hashlib and Python integers)
over ONE oracle pairing per round, the base of the golden chain's round 7 under its key and, for the rounds
forms, round 8's. Tampered ciphertexts are ordinary data to every kernel: nothing here provokes a fault. Every
call is a few items. Every test puts the switch back to 0."""
import contextlib
import ctypes

import pytest

from drand_amd import _lib, callers
from oracle import bls12381 as O
from tests.support import tauth_ref as A
from tests.support import tlock_ref as T

pytestmark = pytest.mark.gpu

ROUND, ROUND_B = 7, 8
GUARD = 64
KDF = _lib.KDF_SHA256_CTR
AUTH = _lib.REJ_TLOCK_AUTH
INF_U = b"\xc0" + bytes(47)
INF_SIG = b"\xc0" + bytes(95)


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def sig(sigs):
    return sigs[ROUND]


@pytest.fixture(scope="module")
def pk(golden):
    return bytes.fromhex(golden["chained"]["pk"])


@pytest.fixture(scope="module")
def ref(sig):
    """ref(mlen) -> three reference items (seed, msg, k, U, V, W) under round 7 at that length, computed once per
    length and never modified. One pairing."""
    fb = A.FixedBase(T.gt_base(O.g2_decompress(sig, check_subgroup=False)))
    cache = {}

    def get(mlen):
        if mlen not in cache:
            cache[mlen] = tuple(A.batch(fb, 3, mlen))
        return cache[mlen]
    return get


@pytest.fixture(scope="module")
def ref_b(sigs):
    """One reference item (seed, msg, k, U, V, W) under round 8 at mlen 33: the second pairing, for the rounds forms."""
    base = T.gt_base(O.g2_decompress(sigs[ROUND_B], check_subgroup=False))
    seed, msg = A.seed_of(77), A.message(77, 33)
    return (seed, msg, A.h3(seed, msg)) + A.encrypt(base, seed, msg)


def col(items, k):
    return [it[k] for it in items]


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


class Guarded:
    """nbytes of 0xAA between two guards of 64 bytes of 0xAA."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = (ctypes.c_uint8 * (nbytes + 2 * GUARD))(*([0xAA] * (nbytes + 2 * GUARD)))
        self.ptr = ctypes.cast(ctypes.byref(self.buf, GUARD), _lib.u8p)

    def bytes(self):
        raw = bytes(self.buf)
        assert raw[:GUARD] == b"\xaa" * GUARD and raw[GUARD + self.n:] == b"\xaa" * GUARD, "a guard was written"
        return raw[GUARD:GUARD + self.n]

    def items(self, size):
        b = self.bytes()
        return [b[size * i:size * i + size] for i in range(self.n // size)]

    def untouched(self):
        return self.bytes() == b"\xaa" * self.n


def raw_encrypt(engine, pk, seeds, msgs, mlen, rounds=None):
    """blsv_tlock_encrypt_auth (or _rounds) over guarded outputs: (rc, us, vs, ws, ok)."""
    n = len(seeds)
    us, vs, ws, ok = Guarded(n * 48), Guarded(n * 32), Guarded(n * mlen), Guarded(n)
    if rounds is None:
        rc = engine.lib.blsv_tlock_encrypt_auth(engine.handle, _lib.buf(pk), ROUND, _lib.buf(b"".join(seeds)),
                                                _lib.buf(b"".join(msgs)), mlen, n, KDF, us.ptr, vs.ptr, ws.ptr, ok.ptr)
    else:
        rc = engine.lib.blsv_tlock_encrypt_auth_rounds(engine.handle, _lib.buf(pk), (ctypes.c_uint64 * n)(*rounds),
                                                       _lib.buf(b"".join(seeds)), _lib.buf(b"".join(msgs)), mlen, n, KDF,
                                                       us.ptr, vs.ptr, ws.ptr, ok.ptr)
    return rc, us, vs, ws, ok


def raw_decrypt(engine, sig, us, vs, ws, mlen):
    """blsv_tlock_decrypt_auth over guarded outputs: (rc, sig_class, out, ok, classes)."""
    n = len(us)
    out, ok, cls, sc = Guarded(n * mlen), Guarded(n), Guarded(n), Guarded(1)
    rc = engine.lib.blsv_tlock_decrypt_auth(engine.handle, _lib.buf(sig), _lib.buf(b"".join(us)), _lib.buf(b"".join(vs)),
                                            _lib.buf(b"".join(ws)), mlen, n, KDF, out.ptr, ok.ptr, cls.ptr, sc.ptr)
    return rc, sc, out, ok, cls


def raw_decrypt_rounds(engine, sig_list, counts, us, vs, ws, mlen):
    """blsv_tlock_decrypt_auth_rounds over guarded outputs: (rc, sig classes, out, ok, classes)."""
    n, m = len(us), len(sig_list)
    out, ok, cls, sc = Guarded(n * mlen), Guarded(n), Guarded(n), Guarded(m)
    rc = engine.lib.blsv_tlock_decrypt_auth_rounds(engine.handle, _lib.buf(b"".join(sig_list)), (ctypes.c_uint64 * m)(*counts), m,
                                                   _lib.buf(b"".join(us)), _lib.buf(b"".join(vs)), _lib.buf(b"".join(ws)), mlen,
                                                   n, KDF, out.ptr, ok.ptr, cls.ptr, sc.ptr)
    return rc, sc, out, ok, cls


@contextlib.contextmanager
def lat(engine, open_items=0, seal_items=0):
    engine.set_tauth_lat_max(open_items, seal_items)
    try:
        yield
    finally:
        engine.set_tauth_lat_max(0, 0)


def others(engine):
    """every counter a routed call must leave alone"""
    return (engine.tlock_stats(), engine.tlock_open_rounds_stats(), engine.tlock_seal_stats(),
            engine.tlock_seal_rounds_stats()[1], engine.tlock_lat_stats(), engine.tseal_lat_stats())


def test_switch_is_its_own_keeps_and_clamps(engine):
    try:
        assert engine.set_tauth_lat_max(3, 5) == 5
        assert engine.set_tauth_lat_max(None, 2) == 3 and engine.set_tauth_lat_max(1, None) == 2, "None keeps"
        prev = engine.set_chunk(16384)
        try:
            assert engine.set_tauth_lat_max(10 ** 9, 10 ** 9) == 16384, "clamped to the chunk"
        finally:
            engine.set_chunk(prev)
    finally:
        assert engine.set_tauth_lat_max(0, 0) == 0


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("n,mlen", [(3, m) for m in A.MLENS] + [(1, 32)])
def test_encrypt_values(engine, pk, ref, n, mlen):
    items = ref(mlen)[:n]
    c0, o0 = engine.tauth_lat_stats(), others(engine)
    with lat(engine, seal_items=4):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1), mlen)
    assert rc == 0 and ok.bytes() == b"\x01" * n
    assert us.items(48) == col(items, 3) and vs.items(32) == col(items, 4) and ws.items(mlen) == col(items, 5)
    c1 = engine.tauth_lat_stats()
    assert c1 == (c0[0], c0[1], c0[2] + 1, c0[3] + n) and others(engine) == o0


def test_encrypt_rounds_values(engine, pk, ref, ref_b):
    """Three items to the rounds 7, 8, 7 (two distinct rounds: one more oracle base) through the rounds form."""
    mlen = 33
    items = [ref(mlen)[0], ref_b, ref(mlen)[2]]
    c0, o0 = engine.tauth_lat_stats(), others(engine)
    with lat(engine, seal_items=4):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1), mlen, rounds=[ROUND, ROUND_B, ROUND])
        res = engine.tlock_encrypt_auth_rounds([ROUND_B], [ref_b[0]], [ref_b[1]], pk48=pk)
    assert rc == 0 and ok.bytes() == b"\x01" * 3
    assert us.items(48) == col(items, 3) and vs.items(32) == col(items, 4) and ws.items(mlen) == col(items, 5)
    assert res.ok == [True] and (res.us, res.vs, res.ws) == ([ref_b[3]], [ref_b[4]], [ref_b[5]])
    assert engine.tauth_lat_stats() == (c0[0], c0[1], c0[2] + 2, c0[3] + 4) and others(engine) == o0


@pytest.mark.parametrize("n,mlen", [(3, m) for m in A.MLENS] + [(1, 32)])
def test_decrypt_values(engine, sig, ref, n, mlen):
    items = ref(mlen)[:n]
    c0, o0 = engine.tauth_lat_stats(), others(engine)
    with lat(engine, open_items=4):
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(items, 3), col(items, 4), col(items, 5), mlen)
    assert rc == 0 and sc.bytes() == b"\x00"
    assert ok.bytes() == b"\x01" * n and cls.bytes() == bytes(n) and out.items(mlen) == col(items, 1)
    assert engine.tauth_lat_stats() == (c0[0] + 1, c0[1] + n, c0[2], c0[3]) and others(engine) == o0


def test_decrypt_rounds_values(engine, sigs, ref, ref_b):
    mlen = 33
    items = [ref(mlen)[0], ref(mlen)[1], ref_b]
    c0, o0 = engine.tauth_lat_stats(), others(engine)
    with lat(engine, open_items=4):
        rc, sc, out, ok, cls = raw_decrypt_rounds(engine, [sigs[ROUND], sigs[ROUND_B]], [2, 1], col(items, 3), col(items, 4),
                                                  col(items, 5), mlen)
        res = engine.tlock_decrypt_auth_rounds([sigs[ROUND], sigs[ROUND_B]], [col(items[:2], 3), [ref_b[3]]],
                                               [col(items[:2], 4), [ref_b[4]]], [col(items[:2], 5), [ref_b[5]]])
    assert rc == 0 and sc.bytes() == bytes(2) and ok.bytes() == b"\x01" * 3 and cls.bytes() == bytes(3)
    assert out.items(mlen) == col(items, 1)
    assert res.msgs == col(items, 1) and res.sig_class == [0, 0] and res.reject_class == [0, 0, 0]
    assert engine.tauth_lat_stats() == (c0[0] + 2, c0[1] + 6, c0[2], c0[3]) and others(engine) == o0


# ------------------------------------------------------------------ rejects
def test_decrypt_rejects(engine, sigs, sig, ref):
    mlen = 33
    a, b, c = ref(mlen)
    good = [a, b, c, a]
    us, vs, ws = col(good, 3), col(good, 4), col(good, 5)
    vs[1] = flip(vs[1], 9, 0x04)
    us[2] = a[3]  # another item's valid U
    us[3] = INF_U
    c0 = engine.tauth_lat_stats()
    with lat(engine, open_items=4):
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, us, vs, ws, mlen)
        assert rc == 0 and sc.bytes() == b"\x00"
        assert cls.bytes() == bytes([0, AUTH, AUTH, AUTH]) and ok.bytes() == bytes([1, 0, 0, 0])
        assert out.items(mlen) == [a[1]] + [bytes(mlen)] * 3
        us, vs, ws = col(good, 3), col(good, 4), col(good, 5)
        for s in (sigs[ROUND_B], INF_SIG):  # a valid signature of the wrong round; sigma at infinity
            rc, sc, out, ok, cls = raw_decrypt(engine, s, us, vs, ws, mlen)
            assert rc == 0 and sc.bytes() == b"\x00"
            assert cls.bytes() == bytes([AUTH] * 4) and ok.bytes() == bytes(4) and out.bytes() == bytes(4 * mlen)
        off = T.bad_us()[O.REJ_NOT_ON_CURVE]
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, [off], vs[:1], ws[:1], mlen)
        assert rc == 0 and cls.bytes() == bytes([O.REJ_NOT_ON_CURVE]) and ok.bytes() == b"\x00" and out.bytes() == bytes(mlen)
        assert engine.tauth_lat_stats()[:2] == (c0[0] + 4, c0[1] + 13)
        # a sigma that does not decode: BLSV_EINVAL with its class, and no per-item output touched
        bad_cls, bad = sorted(T.bad_sigs(sig).items())[0]
        rc, sc, out, ok, cls = raw_decrypt(engine, bad, us, vs, ws, mlen)
        assert rc == _lib.BLSV_EINVAL and sc.bytes() == bytes([bad_cls])
        assert out.untouched() and ok.untouched() and cls.untouched()
        # the rounds form: that round's items only; and an item-less bad signature gets its class (the idle workgroup)
        rc, sc, out, ok, cls = raw_decrypt_rounds(engine, [bad, sig, bad], [1, 3, 0], us, vs, ws, mlen)
        assert rc == 0 and sc.bytes() == bytes([bad_cls, 0, bad_cls])
        assert cls.bytes() == bytes([_lib.REJ_TLOCK_SIG, 0, 0, 0]) and ok.bytes() == bytes([0, 1, 1, 1])
        assert out.items(mlen) == [bytes(mlen), b[1], c[1], a[1]]
        # U's own decode class comes before the signature's
        rc, sc, out, ok, cls = raw_decrypt_rounds(engine, [bad], [1], [off], vs[:1], ws[:1], mlen)
        assert rc == 0 and sc.bytes() == bytes([bad_cls]) and cls.bytes() == bytes([O.REJ_NOT_ON_CURVE])
    assert engine.tauth_lat_stats()[:2] == (c0[0] + 7, c0[1] + 22)


# ------------------------------------------------------------------ routing
def test_routing_edge(engine, sig, pk, ref):
    """L = 4: n = 4 routes and n = 5 does not; both give the bytes of the same call with the switch at 0 (a second
    check beside the reference, which the 4 and 5 items drawn cyclically from the three also meet)."""
    mlen = 13
    items = [ref(mlen)[i % 3] for i in range(5)]
    us, vs, ws = col(items, 3), col(items, 4), col(items, 5)
    vs[1] = flip(vs[1], 0, 0x80)

    def both(n):
        e = raw_encrypt(engine, pk, col(items[:n], 0), col(items[:n], 1), mlen)
        d = raw_decrypt(engine, sig, us[:n], vs[:n], ws[:n], mlen)
        assert e[0] == 0 and d[0] == 0
        return [x.bytes() for x in e[1:]], [x.bytes() for x in d[1:]]
    off = {n: both(n) for n in (4, 5)}
    for n in (4, 5):
        t0, l0, s0 = engine.tauth_lat_stats(), engine.tlock_stats()[1], engine.tlock_seal_stats()[1]
        with lat(engine, 4, 4):
            on = both(n)
        assert on == off[n]
        assert on[0][:3] == [b"".join(col(items[:n], k)) for k in (3, 4, 5)] and on[0][3] == b"\x01" * n
        assert on[1][3] == bytes(AUTH if i == 1 else 0 for i in range(n))
        t1, l1, s1 = engine.tauth_lat_stats(), engine.tlock_stats()[1], engine.tlock_seal_stats()[1]
        if n == 4:
            assert t1 == (t0[0] + 1, t0[1] + 4, t0[2] + 1, t0[3] + 4) and (l1, s1) == (l0, s0)
        else:
            assert t1 == t0 and (l1, s1) == (l0 + 5, s0 + 5)


def test_rounds_decrypt_routes_only_while_the_plan_accepts(engine, sigs, sig, ref):
    """L = 2 and three signatures without items: more idle workgroups than L, so the call takes the batch path."""
    mlen = 4
    it = ref(mlen)[0]
    t0 = engine.tauth_lat_stats()
    with lat(engine, open_items=2):
        res = engine.tlock_decrypt_auth_rounds([sig] + [sigs[ROUND_B]] * 3, [[it[3]], [], [], []], [[it[4]], [], [], []],
                                               [[it[5]], [], [], []])
        assert res.msgs == [it[1]] and engine.tauth_lat_stats() == t0
        res = engine.tlock_decrypt_auth_rounds([sig] + [sigs[ROUND_B]] * 2, [[it[3]], [], []], [[it[4]], [], []], [[it[5]], [], []])
        assert res.msgs == [it[1]] and res.sig_class == [0, 0, 0] and engine.tauth_lat_stats()[:2] == (t0[0] + 1, t0[1] + 1)


def test_dev_forms_never_route(engine, sig, pk, ref):
    import torch
    mlen = 32
    items = ref(mlen)[:2]
    dev = torch.device("cuda", 0)

    def up(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_us, d_vs, d_ws = up(b"".join(col(items, 3))), up(b"".join(col(items, 4))), up(b"".join(col(items, 5)))
    d_seeds, d_msgs = up(b"".join(col(items, 0))), up(b"".join(col(items, 1)))
    d_out, d_cls = torch.zeros(2 * mlen, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
    d_u, d_v = torch.zeros(96, dtype=torch.uint8, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    d_w, d_ok = torch.zeros(2 * mlen, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    t0 = engine.tauth_lat_stats()
    with lat(engine, 4, 4):
        engine.tlock_decrypt_auth_dev(sig, d_us.data_ptr(), d_vs.data_ptr(), d_ws.data_ptr(), mlen, 2, d_out.data_ptr(),
                                      d_cls.data_ptr())
        engine.tlock_encrypt_auth_dev(ROUND, d_seeds.data_ptr(), d_msgs.data_ptr(), mlen, 2, d_u.data_ptr(), d_v.data_ptr(),
                                      d_w.data_ptr(), d_ok.data_ptr(), pk48=pk)
        engine.synchronize()
    assert engine.tauth_lat_stats() == t0
    assert bytes(d_out.cpu().numpy()) == b"".join(col(items, 1)) and bytes(d_cls.cpu().numpy()) == bytes(2)
    assert bytes(d_u.cpu().numpy()) == b"".join(col(items, 3)) and bytes(d_w.cpu().numpy()) == b"".join(col(items, 5))


# ------------------------------------------------------------------ caches
def test_caches_survive_routed_calls(engine, sigs, sig, pk, ref):
    mlen = 32
    items = ref(mlen)
    # the batch path's caches hold (sigma_7) and (pk, round 7) after these two calls
    assert engine.tlock_decrypt_auth(sig, col(items, 3), col(items, 4), col(items, 5)).msgs == col(items, 1)
    assert engine.tlock_encrypt_auth(ROUND, col(items, 0), col(items, 1), pk48=pk).us == col(items, 3)
    prepared, bases = engine.tlock_stats()[0], engine.tlock_seal_stats()[0]
    with lat(engine, 4, 4):  # routed calls under ANOTHER signature and to ANOTHER round
        assert engine.tlock_decrypt_auth(sigs[ROUND_B], col(items, 3), col(items, 4), col(items, 5)).msgs == [None] * 3
        assert engine.tlock_encrypt_auth(ROUND_B, col(items, 0), col(items, 1), pk48=pk).ok == [True] * 3
    assert (engine.tlock_stats()[0], engine.tlock_seal_stats()[0]) == (prepared, bases)
    # ... and the following batch calls hit their caches
    assert engine.tlock_decrypt_auth(sig, col(items, 3), col(items, 4), col(items, 5)).msgs == col(items, 1)
    assert engine.tlock_encrypt_auth(ROUND, col(items, 0), col(items, 1), pk48=pk).us == col(items, 3)
    assert (engine.tlock_stats()[0], engine.tlock_seal_stats()[0]) == (prepared, bases)


# ------------------------------------------------------------------ the callers
def test_callers_round_trip_on_the_latency_path(engine, sigs, pk):
    engine.set_public_key(pk)
    msgs = [b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100))]
    t0 = engine.tauth_lat_stats()
    with lat(engine, 4, 4):
        cts = callers.timelock_encrypt_auth(engine, ROUND, msgs)  # fresh seeds; one call per message length
        assert callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND], cts) == msgs
        assert callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND_B], cts) == [None] * 3
    t1 = engine.tauth_lat_stats()
    assert t1[1] == t0[1] + 6 and t1[3] == t0[3] + 3, "every call took the latency path"
