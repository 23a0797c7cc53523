"""The authenticated timelock on the GPU (blsv_tlock_encrypt_auth* / blsv_tlock_decrypt_auth*,
drand_amd/csrc/k_tauth.hip): the four timelock passes with the Fujisaki-Okamoto tail on the device.

Expected bytes never come from the code under test: tests/support/tauth_ref.py (hashlib and Python integers)
over ONE oracle pairing for the module, the base of the golden chain's round 7 under its key. Tampered
ciphertexts are ordinary data to every kernel: nothing here provokes a fault.
Shapes: the 65-item batch (21 / 22 / 63: the 3-lane final exponentiation; 64 / 65: the one-lane kernels' wave
edge); the lengths of tauth_ref.MLENS, at which the hashing can go wrong (the hashed length is 52 + mlen).
"""
import ctypes

import pytest

from drand_amd import _lib, callers
from oracle import bls12381 as O
from tests.support import tauth_ref as A
from tests.support import tlock_ref as T

pytestmark = pytest.mark.gpu

ROUND = 7
N = 65
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
    """ref(mlen) -> the 65 reference items (seed, msg, k, U, V, W) at that length, computed once per length and
    never modified. One pairing for the module."""
    fb = A.FixedBase(T.gt_base(O.g2_decompress(sig, check_subgroup=False)))
    cache = {}

    def get(mlen):
        if mlen not in cache:
            cache[mlen] = tuple(A.batch(fb, N, mlen))
        return cache[mlen]
    return get


def col(items, k):
    return [it[k] for it in items]


class Guarded:
    """nbytes of 0xAA (or `fill`) between two guards of 64 bytes of 0xAA."""

    def __init__(self, nbytes, fill=None):
        self.n = nbytes
        self.buf = (ctypes.c_uint8 * (nbytes + 2 * GUARD))(*([0xAA] * (nbytes + 2 * GUARD)))
        if fill is not None:
            ctypes.memmove(ctypes.byref(self.buf, GUARD), fill, nbytes)
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


def ptr_of(x):
    return x.ptr if isinstance(x, Guarded) else _lib.buf(b"".join(x))


def raw_encrypt(engine, pk, seeds, msgs, mlen, kdf=KDF, out=None, rounds=None):
    """blsv_tlock_encrypt_auth (or _rounds) over guarded outputs: (rc, us, vs, ws, ok)."""
    n = len(seeds)
    us, vs, ok = Guarded(n * 48), Guarded(n * 32), Guarded(n)
    ws = out or Guarded(n * mlen)
    if rounds is None:
        rc = engine.lib.blsv_tlock_encrypt_auth(engine.handle, _lib.buf(pk), ROUND, ptr_of(seeds), ptr_of(msgs), mlen, n, kdf,
                                                us.ptr, vs.ptr, ws.ptr, ok.ptr)
    else:
        rc = engine.lib.blsv_tlock_encrypt_auth_rounds(engine.handle, _lib.buf(pk), (ctypes.c_uint64 * n)(*rounds),
                                                       ptr_of(seeds), ptr_of(msgs), mlen, n, kdf, us.ptr, vs.ptr, ws.ptr,
                                                       ok.ptr)
    return rc, us, vs, ws, ok


def raw_decrypt(engine, sig, us, vs, ws, mlen, kdf=KDF, out=None):
    """blsv_tlock_decrypt_auth over guarded outputs: (rc, sig_class, out, ok, classes)."""
    n = len(us)
    out = out or Guarded(n * mlen)
    ok, cls = Guarded(n), Guarded(n)
    sc = ctypes.c_uint8(0xEE)
    rc = engine.lib.blsv_tlock_decrypt_auth(engine.handle, _lib.buf(sig), _lib.buf(b"".join(us)), _lib.buf(b"".join(vs)),
                                            ptr_of(ws), mlen, n, kdf, out.ptr, ok.ptr, cls.ptr,
                                            ctypes.cast(ctypes.byref(sc), _lib.u8p))
    return rc, sc.value, out, ok, cls


SHAPES = [(1, 32), (64, 32), (65, 32)] + [(65, m) for m in A.MLENS if m != 32]


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("n,mlen", SHAPES)
def test_encrypt_auth_values(engine, pk, ref, n, mlen):
    items = ref(mlen)[:n]
    before = engine.tlock_seal_stats()[1]
    rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1), mlen)
    assert rc == 0 and engine.tlock_seal_stats()[1] == before + n, "counted in the pass it runs"
    assert ok.bytes() == b"\x01" * n
    assert us.items(48) == col(items, 3) and vs.items(32) == col(items, 4) and ws.items(mlen) == col(items, 5)
    if mlen == 32:
        assert us.items(48) == engine.tlock_seal(ROUND, col(items, 2), pk48=pk).us
        res = engine.tlock_encrypt_auth(ROUND, col(items, 0), col(items, 1), pk48=pk)
        assert res.ok == [True] * n and (res.us, res.vs, res.ws) == (col(items, 3), col(items, 4), col(items, 5))


@pytest.mark.parametrize("n,mlen", SHAPES)
def test_decrypt_auth_values(engine, sig, ref, n, mlen):
    items = ref(mlen)[:n]
    before = engine.tlock_stats()[1]
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(items, 3), col(items, 4), col(items, 5), mlen)
    assert rc == 0 and sc == 0 and engine.tlock_stats()[1] == before + n, "counted in the pass it runs"
    assert ok.bytes() == b"\x01" * n and cls.bytes() == bytes(n)
    assert out.items(mlen) == col(items, 1)
    res = engine.tlock_decrypt_auth(sig, col(items, 3), col(items, 4), col(items, 5))
    assert res.ok == [True] * n and res.reject_class == [0] * n and res.msgs == col(items, 1)


def test_engine_made_ciphertexts_round_trip(engine, sig, pk):
    msgs = [bytes((3 * i + j) % 256 for j in range(13)) for i in range(N)]
    seeds = [A.seed_of(1000 + i) for i in range(N)]
    enc = engine.tlock_encrypt_auth(ROUND, seeds, msgs, pk48=pk)
    assert enc.ok == [True] * N
    assert engine.tlock_decrypt_auth(sig, enc.us, enc.vs, enc.ws).msgs == msgs


# ------------------------------------------------------------------ tampering
def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


AT = (0, 32, 64)


@pytest.mark.parametrize("case", ["v_bit", "w_first", "w_last", "u_swapped", "u_infinity"])
@pytest.mark.parametrize("mlen", [32, 33])
def test_tampering(engine, sig, ref, case, mlen):
    items = ref(mlen)
    us, vs, ws = col(items, 3), col(items, 4), col(items, 5)
    for i in AT:
        if case == "v_bit":
            vs[i] = flip(vs[i], 9, 0x04)
        elif case == "w_first":
            ws[i] = flip(ws[i], 0)
        elif case == "w_last":
            ws[i] = flip(ws[i], mlen - 1, 0x80)
        elif case == "u_swapped":
            us[i] = items[i + 1 if i < 64 else 5][3]  # another item's valid U
        else:
            us[i] = INF_U
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, us, vs, ws, mlen)
    assert rc == 0 and sc == 0
    assert cls.bytes() == bytes(AUTH if i in AT else 0 for i in range(N))
    assert ok.bytes() == bytes(0 if i in AT else 1 for i in range(N))
    assert out.items(mlen) == [bytes(mlen) if i in AT else items[i][1] for i in range(N)]
    res = engine.tlock_decrypt_auth(sig, us, vs, ws)
    assert [m is None for m in res.msgs] == [i in AT for i in range(N)]


@pytest.mark.parametrize("bad_cls", [2, 3, 4, 5, 6])
def test_u_decode_classes_keep_their_class(engine, sig, ref, bad_cls):
    mlen = 3
    items = ref(mlen)
    us = [T.bad_us()[bad_cls] if i in AT else u for i, u in enumerate(col(items, 3))]
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, us, col(items, 4), col(items, 5), mlen)
    assert rc == 0 and cls.bytes() == bytes(bad_cls if i in AT else 0 for i in range(N))
    assert ok.bytes() == bytes(0 if i in AT else 1 for i in range(N))
    assert out.items(mlen) == [bytes(mlen) if i in AT else items[i][1] for i in range(N)]


def test_wrong_round_signature_and_sigma_at_infinity_fail_every_item(engine, sigs, ref):
    mlen = 32
    items = ref(mlen)
    for s in (sigs[8], INF_SIG):
        rc, sc, out, ok, cls = raw_decrypt(engine, s, col(items, 3), col(items, 4), col(items, 5), mlen)
        assert rc == 0 and sc == 0
        assert cls.bytes() == bytes([AUTH]) * N and ok.bytes() == bytes(N) and out.bytes() == bytes(N * mlen)


def test_bad_sigma_touches_nothing(engine, sig, ref):
    from drand_amd.engine import SignatureRejected
    items = ref(3)[:2]
    for bad_cls, s in sorted(T.bad_sigs(sig).items()):
        rc, sc, out, ok, cls = raw_decrypt(engine, s, col(items, 3), col(items, 4), col(items, 5), 3)
        assert rc == _lib.BLSV_EINVAL and sc == bad_cls
        assert out.untouched() and ok.untouched() and cls.untouched()
        with pytest.raises(SignatureRejected) as ei:
            engine.tlock_decrypt_auth(s, col(items, 3), col(items, 4), col(items, 5))
        assert ei.value.sig_class == bad_cls


@pytest.mark.parametrize("kdf,mlen", [(0, 32), (2, 32), (KDF, 0), (KDF, 257)])
def test_bad_kdf_or_length_is_einval_with_nothing_touched(engine, sig, pk, ref, kdf, mlen):
    width = max(mlen, 1)
    items = ref(3)[:2]
    body = [bytes(width)] * 2
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(items, 3), col(items, 4), body, mlen, kdf=kdf, out=Guarded(2 * width))
    assert rc == _lib.BLSV_EINVAL and sc == 0xEE and out.untouched() and ok.untouched() and cls.untouched()
    for rounds in (None, [ROUND, ROUND + 1]):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), body, mlen, kdf=kdf, out=Guarded(2 * width), rounds=rounds)
        assert rc == _lib.BLSV_EINVAL and us.untouched() and vs.untouched() and ws.untouched() and ok.untouched()
    out, ok, cls, sc = Guarded(2 * width), Guarded(2), Guarded(2), Guarded(1)
    rc = engine.lib.blsv_tlock_decrypt_auth_rounds(engine.handle, _lib.buf(sig), (ctypes.c_uint64 * 1)(2), 1,
                                                   _lib.buf(b"".join(col(items, 3))), _lib.buf(b"".join(col(items, 4))),
                                                   _lib.buf(b"".join(body)), mlen, 2, kdf, out.ptr, ok.ptr, cls.ptr, sc.ptr)
    assert rc == _lib.BLSV_EINVAL and out.untouched() and ok.untouched() and cls.untouched() and sc.untouched()


@pytest.mark.parametrize("mlen", [3, 32])
def test_in_place(engine, sig, pk, ref, mlen):
    items = ref(mlen)
    ws = col(items, 5)
    ws[7] = flip(ws[7], 0)  # a failing item: its bytes become zeros
    buf = Guarded(N * mlen, fill=b"".join(ws))
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(items, 3), col(items, 4), buf, mlen, out=buf)
    assert rc == 0 and out is buf
    assert buf.items(mlen) == [bytes(mlen) if i == 7 else items[i][1] for i in range(N)]
    assert cls.bytes() == bytes(AUTH if i == 7 else 0 for i in range(N))
    buf = Guarded(N * mlen, fill=b"".join(col(items, 1)))
    rc, us, vs, w, ok = raw_encrypt(engine, pk, col(items, 0), buf, mlen, out=buf)
    assert rc == 0 and w is buf and buf.items(mlen) == col(items, 5)
    assert us.items(48) == col(items, 3) and vs.items(32) == col(items, 4)


# ------------------------------------------------------------------ the _dev forms
@pytest.mark.parametrize("mlen,offset", [(32, 0), (3, 1)])
def test_dev_forms(engine, sig, pk, ref, mlen, offset):
    """torch byte tensors: once 4-byte aligned with mlen = 32, once with every pointer offset by one byte and
    mlen = 3; one undecodable U and one tampered V among them. All four _dev entry points."""
    import torch
    items = ref(mlen)
    dev = torch.device("cuda", 0)
    us, vs = col(items, 3), col(items, 4)
    us[5] = T.bad_us()[5]
    vs[9] = flip(vs[9], 31, 0x01)

    def up(data):
        return torch.frombuffer(bytearray(bytes(offset) + data), dtype=torch.uint8).to(dev)

    def fresh(nbytes):
        return torch.full((offset + nbytes + GUARD,), 0xAA, dtype=torch.uint8, device=dev)

    def down(t, nbytes):
        raw = bytes(t.cpu().numpy())
        assert raw[:offset] == b"\xaa" * offset and raw[offset + nbytes:] == b"\xaa" * GUARD, "written out of bounds"
        return raw[offset:offset + nbytes]

    def split(b, k):
        return [b[k * i:k * i + k] for i in range(len(b) // k)]

    d_us, d_vs, d_ws = up(b"".join(us)), up(b"".join(vs)), up(b"".join(col(items, 5)))
    d_out, d_cls = fresh(N * mlen), fresh(N)
    d_out2, d_cls2, d_scls = fresh(N * mlen), fresh(N), fresh(2)
    d_seeds, d_msgs = up(b"".join(col(items, 0))), up(b"".join(col(items, 1)))
    d_u, d_v, d_w, d_ok = fresh(N * 48), fresh(N * 32), fresh(N * mlen), fresh(N)
    d_rounds = torch.tensor([ROUND] * N, dtype=torch.int64, device=dev)
    d_u2, d_v2, d_w2, d_ok2 = fresh(N * 48), fresh(N * 32), fresh(N * mlen), fresh(N)
    torch.cuda.synchronize(dev)  # the fills run on torch's stream, the engine on its own
    p = lambda t: t.data_ptr() + offset
    engine.tlock_decrypt_auth_dev(sig, p(d_us), p(d_vs), p(d_ws), mlen, N, p(d_out), p(d_cls))
    engine.tlock_decrypt_auth_rounds_dev([sig, sig], [1, N - 1], p(d_us), p(d_vs), p(d_ws), mlen, N, p(d_out2), p(d_cls2),
                                         p(d_scls))
    engine.tlock_encrypt_auth_dev(ROUND, p(d_seeds), p(d_msgs), mlen, N, p(d_u), p(d_v), p(d_w), p(d_ok), pk48=pk)
    engine.tlock_encrypt_auth_rounds_dev(d_rounds.data_ptr(), p(d_seeds), p(d_msgs), mlen, N, p(d_u2), p(d_v2), p(d_w2),
                                         p(d_ok2), pk48=pk)
    engine.synchronize()
    torch.cuda.synchronize(dev)
    want = [bytes(mlen) if i in (5, 9) else it[1] for i, it in enumerate(items)]
    want_cls = bytes(5 if i == 5 else AUTH if i == 9 else 0 for i in range(N))
    for o, c in ((d_out, d_cls), (d_out2, d_cls2)):
        assert split(down(o, N * mlen), mlen) == want and down(c, N) == want_cls
    assert down(d_scls, 2) == bytes(2)
    for u, v, w, ok in ((d_u, d_v, d_w, d_ok), (d_u2, d_v2, d_w2, d_ok2)):
        assert split(down(u, N * 48), 48) == col(items, 3) and split(down(v, N * 32), 32) == col(items, 4)
        assert split(down(w, N * mlen), mlen) == col(items, 5) and down(ok, N) == b"\x01" * N


def test_dev_forms_require_the_class_buffer(engine, sig, ref):
    import torch
    items = ref(3)[:2]
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(256, dtype=torch.uint8, device=dev)
    d_out = torch.full((64,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    a = d_in.data_ptr()
    rc = engine.lib.blsv_tlock_decrypt_auth_dev(engine.handle, _lib.buf(sig), a, a + 96, a + 160, 3, 2, KDF, d_out.data_ptr(),
                                                None, None)
    assert rc == _lib.BLSV_EINVAL
    rc = engine.lib.blsv_tlock_decrypt_auth_rounds_dev(engine.handle, _lib.buf(sig), (ctypes.c_uint64 * 1)(2), 1, a, a + 96,
                                                       a + 160, 3, 2, KDF, d_out.data_ptr(), None, None, None)
    assert rc == _lib.BLSV_EINVAL
    engine.synchronize()
    assert bytes(d_out.cpu().numpy()) == b"\xaa" * 64


# ------------------------------------------------------------------ the rounds forms
def test_decrypt_auth_rounds(engine, sigs, sig, ref):
    """Three signatures with counts 0, 1 and 66; then the middle one corrupted; then a valid one of the wrong round."""
    mlen = 32
    items = ref(mlen)
    idx = [i % N for i in range(67)]
    us, vs, ws = ([items[k][c] for k in idx] for c in (3, 4, 5))
    want = [items[k][1] for k in idx]
    runs = lambda xs: [[], xs[:1], xs[1:]]
    before = engine.tlock_open_rounds_stats()[1]
    res = engine.tlock_decrypt_auth_rounds([sigs[8], sig, sig], runs(us), runs(vs), runs(ws))
    assert engine.tlock_open_rounds_stats()[1] == before + 67, "counted in the pass it runs"
    assert res.ok == [True] * 67 and res.reject_class == [0] * 67 and res.sig_class == [0, 0, 0] and res.msgs == want
    bad_cls, bad = sorted(T.bad_sigs(sig).items())[0]
    res = engine.tlock_decrypt_auth_rounds([sigs[8], bad, sig], runs(us), runs(vs), runs(ws))
    assert res.sig_class == [0, bad_cls, 0]
    assert res.reject_class == [_lib.REJ_TLOCK_SIG] + [0] * 66 and res.msgs == [None] + want[1:]
    res = engine.tlock_decrypt_auth_rounds([sigs[8], sigs[8], sig], runs(us), runs(vs), runs(ws))
    assert res.sig_class == [0, 0, 0]
    assert res.reject_class == [AUTH] + [0] * 66 and res.ok == [False] + [True] * 66 and res.msgs == [None] + want[1:]
    # ... and the failing item's bytes are zeros, with the guards intact
    out, ok, cls, sc = Guarded(67 * mlen), Guarded(67), Guarded(67), Guarded(3)
    rc = engine.lib.blsv_tlock_decrypt_auth_rounds(engine.handle, _lib.buf(sigs[8] + sigs[8] + sig),
                                                   (ctypes.c_uint64 * 3)(0, 1, 66), 3, _lib.buf(b"".join(us)),
                                                   _lib.buf(b"".join(vs)), _lib.buf(b"".join(ws)), mlen, 67, KDF, out.ptr,
                                                   ok.ptr, cls.ptr, sc.ptr)
    assert rc == 0 and out.items(mlen) == [bytes(mlen)] + want[1:] and sc.bytes() == bytes(3)
    assert cls.bytes() == bytes([AUTH] + [0] * 66) and ok.bytes() == bytes([0] + [1] * 66)


def test_encrypt_auth_rounds(engine, pk, sig, ref):
    """64 distinct rounds: U and K are consistent with blsv_tlock_seal_rounds for the derived scalars (pinned by
    its own tests); the item locked to ROUND is checked against the reference."""
    mlen = 33
    items = ref(mlen)[:64]
    rounds = [ROUND + i for i in range(64)]
    sealed = engine.tlock_seal_rounds(rounds, col(items, 2), pk48=pk)
    before = engine.tlock_seal_rounds_stats()[1]
    rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1), mlen, rounds=rounds)
    assert rc == 0 and engine.tlock_seal_rounds_stats()[1] == before + 64, "counted in the pass it runs"
    assert ok.bytes() == b"\x01" * 64 and us.items(48) == sealed.us == col(items, 3)
    assert vs.items(32) == [A.seal_tail(it[0], it[1], g)[0] for it, g in zip(items, sealed.gt)]
    assert ws.items(mlen) == [A.seal_tail(it[0], it[1], g)[1] for it, g in zip(items, sealed.gt)]
    assert (us.items(48)[0], vs.items(32)[0], ws.items(mlen)[0]) == items[0][3:6]
    assert len(set(sealed.gt)) == 64
    res = engine.tlock_encrypt_auth_rounds(rounds, col(items, 0), col(items, 1), pk48=pk)
    assert (res.us, res.vs, res.ws) == (us.items(48), vs.items(32), ws.items(mlen))
    # the ROUND item opens under ROUND's signature
    assert engine.tlock_decrypt_auth(sig, res.us[:1], res.vs[:1], res.ws[:1]).msgs == [items[0][1]]


def test_pass_boundary(engine, sig, pk, ref):
    """n = chunk + 1 with the chunk capped at 16,384: two passes, every item checked; one tampered item on each
    side of the boundary. The items are drawn cyclically from the 65."""
    n, mlen = 16385, 3
    items = ref(mlen)
    idx = [i % N for i in range(n)]
    us, vs, ws = ([items[k][c] for k in idx] for c in (3, 4, 5))
    bad = (16383, 16384)
    for i in bad:
        vs[i] = flip(vs[i], 0, 0x80)
    prev = engine.set_chunk(16384)
    try:
        res = engine.tlock_decrypt_auth(sig, us, vs, ws)
        rres = engine.tlock_decrypt_auth_rounds([sig, sig], [us[:16000], us[16000:]], [vs[:16000], vs[16000:]],
                                                [ws[:16000], ws[16000:]])
        enc = engine.tlock_encrypt_auth(ROUND, [items[k][0] for k in idx], [items[k][1] for k in idx], pk48=pk)
    finally:
        engine.set_chunk(prev)
    want = [None if i in bad else items[k][1] for i, k in enumerate(idx)]
    want_cls = [AUTH if i in bad else 0 for i in range(n)]
    assert res.msgs == want and res.reject_class == want_cls
    assert rres.msgs == want and rres.reject_class == want_cls and rres.sig_class == [0, 0]
    assert enc.ok == [True] * n
    assert (enc.us, enc.vs, enc.ws) == tuple([items[k][c] for k in idx] for c in (3, 4, 5))


# ------------------------------------------------------------------ what must not move
def test_existing_entry_points_and_counters_are_unchanged(engine, sig, sigs, pk, ref):
    """tlock_decrypt / tlock_encrypt give the same bytes before and after authenticated calls on the same context,
    the counters of the other paths do not move, and the sigma and base caches survive a call that uses them."""
    items = ref(32)[:5]
    ks, msgs = [3, 5, 7, 11, O.R - 2], col(items, 1)
    enc0 = engine.tlock_encrypt(ROUND, ks, msgs, pk48=pk)
    dec0 = engine.tlock_decrypt(sig, enc0.us, enc0.cs)
    assert dec0.msgs == msgs

    def counters():
        return (engine.tlock_stats(), engine.tlock_open_rounds_stats(), engine.tlock_seal_stats(),
                engine.tlock_seal_rounds_stats(), engine.tlock_lat_stats(), engine.tseal_lat_stats())
    c0 = counters()
    engine.set_tlock_lat_max(4)
    engine.set_tseal_lat_max(4)
    try:  # the authenticated host forms take the batch path whatever the switches say
        enc = engine.tlock_encrypt_auth(ROUND, col(items, 0), msgs, pk48=pk)
        dec = engine.tlock_decrypt_auth(sig, enc.us, enc.vs, enc.ws)
    finally:
        engine.set_tlock_lat_max(0)
        engine.set_tseal_lat_max(0)
    assert dec.msgs == msgs and (enc.us, enc.vs, enc.ws) == (col(items, 3), col(items, 4), col(items, 5))
    c1 = counters()
    # sigma and (key, round) were cached by the calls above: nothing was prepared or built again
    assert c1[0] == (c0[0][0], c0[0][1] + 5) and c1[2] == (c0[2][0], c0[2][1] + 5)
    assert c1[1] == c0[1] and c1[3] == c0[3] and c1[4] == c0[4] and c1[5] == c0[5]
    assert engine.tlock_encrypt(ROUND, ks, msgs, pk48=pk) == enc0
    assert engine.tlock_decrypt(sig, enc0.us, enc0.cs) == dec0
    assert counters()[0][0] == c0[0][0] and counters()[2][0] == c0[2][0]


# ------------------------------------------------------------------ the callers, end to end
def test_callers_round_trip_and_a_wrong_signature_gives_none(engine, sigs, pk):
    engine.set_public_key(pk)
    msgs = [b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100)), bytes(range(200, 233)), b"\x02"]
    cts = callers.timelock_encrypt_auth(engine, ROUND, msgs)  # fresh seeds, the group key
    assert [(len(u), len(v), len(w)) for u, v, w in cts] == [(48, 32, len(m)) for m in msgs]
    assert callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND], cts) == msgs
    assert callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND], cts, verify=True) == msgs
    assert callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND + 1], cts) == [None] * len(msgs)  # no exception
    with pytest.raises(callers.VerifyError):
        callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND + 1], cts, verify=True)
    tampered = list(cts)
    tampered[2] = (cts[2][0], cts[2][1], flip(cts[2][2], 50))
    assert callers.timelock_decrypt_auth(engine, ROUND, sigs[ROUND], tampered) == msgs[:2] + [None] + msgs[3:]
    cts_r = callers.timelock_encrypt_auth_rounds(engine, [(ROUND, m) for m in msgs[:2]] + [(ROUND + 1, m) for m in msgs[2:]])
    runs = [(ROUND, sigs[ROUND], cts_r[:2]), (ROUND + 1, sigs[ROUND + 1], cts_r[2:])]
    assert callers.timelock_decrypt_auth_rounds(engine, runs) == [msgs[:2], msgs[2:]]
    swapped = [(ROUND, sigs[ROUND + 1], cts_r[:2]), (ROUND + 1, sigs[ROUND + 1], cts_r[2:])]
    assert callers.timelock_decrypt_auth_rounds(engine, swapped) == [[None, None], msgs[2:]]
