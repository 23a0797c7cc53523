"""Timelock encrypt / decrypt in one call on the GPU (blsv_tlock_decrypt* / blsv_tlock_encrypt*,
drand_amd/csrc/k_tmask.hip): the four timelock passes with the key stream and the XOR fused on the device.

Expected bytes never come from the code under test: K = gt_pow(base, r) from ONE oracle pairing for the
module (tests/support/tlock_ref.py; the golden chain's round-7 SignatureV2 is sk * H(MessageV2(7)), so
e(G1, sigma)^3 is the sealing base of (pk, 7) too), and m XOR callers.kdf_sha256_ctr(encode_gt(K), mlen).
Where a whole call is compared with the entry point it fuses (blsv_tlock_open*, blsv_tlock_seal*), that entry
point is pinned by its own test module.
Shapes: the 65-item batch of test_gpu_tlock.py with its full-width scalars (21 / 22 / 63: the 3-lane final
exponentiation; 64 / 65: the one-lane kernels); mlen on both sides of a key-stream block and at the cap, one
multiple of 4 (dword stores) and odd ones (byte stores); the pass boundary is the context chunk.
"""
import ctypes

import pytest

from drand_amd import _lib, callers
from oracle import bls12381 as O
from tests.support import tlock_ref as T

pytestmark = pytest.mark.gpu

ROUND = 7
N = 65
WIDE = (0, 10, 20, 21, 22, 62, 63, 64)  # the items with full-width scalars
GUARD = 64
KDF = _lib.KDF_SHA256_CTR


def scalar(i):
    if i in WIDE:
        return (0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD * (i + 3) + i) % O.R
    return i + 2


def message(i, mlen):
    return bytes((29 * i + 13 * j + 7) % 256 for j in range(mlen))


def xor(a, b):
    assert len(a) == len(b)
    return bytes(x ^ y for x, y in zip(a, b))


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
def base(sig):
    return T.gt_base(O.g2_decompress(sig, check_subgroup=False))  # the module's one pairing


@pytest.fixture(scope="module")
def batch(base):
    """(scalars, us, encoded Gt values) of the 65-item batch, computed once and never modified."""
    rs = [scalar(i) for i in range(N)]
    return rs, [T.u_of(r) for r in rs], [T.encode_gt(T.gt_pow(base, r)) for r in rs]


def masked(gts, msgs):
    return [xor(m, callers.kdf_sha256_ctr(g, len(m))) for g, m in zip(gts, msgs)]


class Guarded:
    """nbytes of 0xAA between two guards of 64 bytes of 0xAA."""

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

    def items(self, mlen):
        b = self.bytes()
        return [b[mlen * i:mlen * i + mlen] for i in range(self.n // mlen)]


def raw_decrypt(engine, sig, us, cs, mlen, kdf=KDF, out=None):
    """blsv_tlock_decrypt over guarded outputs: (rc, sig_class, out, ok, classes)."""
    n = len(us)
    out = out or Guarded(n * mlen)
    ok, cls = Guarded(n), Guarded(n)
    sc = ctypes.c_uint8(0xEE)
    cs_ptr = cs.ptr if isinstance(cs, Guarded) else _lib.buf(b"".join(cs))
    rc = engine.lib.blsv_tlock_decrypt(engine.handle, _lib.buf(sig), _lib.buf(b"".join(us)), cs_ptr, mlen, n, kdf,
                                       out.ptr, ok.ptr, cls.ptr, ctypes.cast(ctypes.byref(sc), _lib.u8p))
    return rc, sc.value, out, ok, cls


def raw_encrypt(engine, pk, scalars, msgs, mlen, kdf=KDF, out=None, rounds=None):
    """blsv_tlock_encrypt (or _rounds) over guarded outputs: (rc, us, cs, ok)."""
    n = len(scalars)
    us, ok = Guarded(n * 48), Guarded(n)
    out = out or Guarded(n * mlen)
    sb = _lib.buf(b"".join(int(k).to_bytes(32, "big") for k in scalars))
    ms_ptr = msgs.ptr if isinstance(msgs, Guarded) else _lib.buf(b"".join(msgs))
    if rounds is None:
        rc = engine.lib.blsv_tlock_encrypt(engine.handle, _lib.buf(pk), ROUND, sb, ms_ptr, mlen, n, kdf, us.ptr, out.ptr,
                                           ok.ptr)
    else:
        rc = engine.lib.blsv_tlock_encrypt_rounds(engine.handle, _lib.buf(pk), (ctypes.c_uint64 * n)(*rounds), sb, ms_ptr,
                                                  mlen, n, kdf, us.ptr, out.ptr, ok.ptr)
    return rc, us, out, ok


# ------------------------------------------------------------------ decrypt
@pytest.mark.parametrize("n,mlen", [(1, 32), (21, 32), (22, 32), (63, 32), (64, 32), (65, 32),
                                    (65, 1), (65, 3), (65, 33), (65, 256)])
def test_decrypt_values(engine, sig, batch, n, mlen):
    _, us, gts = batch
    msgs = [message(i, mlen) for i in range(n)]
    cs = masked(gts[:n], msgs)
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, us[:n], cs, mlen)
    assert rc == 0 and sc == 0
    assert ok.bytes() == b"\x01" * n and cls.bytes() == bytes(n)
    assert out.items(mlen) == msgs
    res = engine.tlock_decrypt(sig, us[:n], cs)
    assert res.ok == [True] * n and res.reject_class == [0] * n and res.msgs == msgs


def test_decrypt_equals_open_then_the_host_kdf(engine, sig, batch):
    """Item by item, U at infinity and sigma at infinity included: both mask with kdf(encode(1))."""
    _, us, gts = batch
    mlen = 33
    mixed = [T.u_of(0)] + us[1:22] + [T.u_of(0)]
    cs = [message(i, mlen) for i in range(23)]
    for s in (sig, b"\xc0" + bytes(95)):
        opened = engine.tlock_open(s, mixed)
        res = engine.tlock_decrypt(s, mixed, cs)
        assert res.ok == opened.ok == [True] * 23 and res.reject_class == opened.reject_class
        assert res.msgs == masked(opened.gt, cs)
    assert engine.tlock_decrypt(sig, mixed, cs).msgs == masked([T.GT_ONE] + gts[1:22] + [T.GT_ONE], cs)
    assert engine.tlock_decrypt(b"\xc0" + bytes(95), mixed, cs).msgs == masked([T.GT_ONE] * 23, cs)


@pytest.mark.parametrize("bad_cls", [2, 3, 4, 5, 6])
def test_decrypt_reject_classes(engine, sig, batch, bad_cls):
    _, us, gts = batch
    mlen = 3
    bad = T.bad_us()[bad_cls]
    at = (0, N // 2, N - 1)
    mixed = [bad if i in at else u for i, u in enumerate(us)]
    cs = [message(i, mlen) for i in range(N)]
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, mixed, cs, mlen)
    assert rc == 0 and sc == 0
    want = masked(gts, cs)
    assert out.items(mlen) == [bytes(mlen) if i in at else want[i] for i in range(N)]
    assert cls.bytes() == bytes(bad_cls if i in at else 0 for i in range(N))
    assert ok.bytes() == bytes(0 if i in at else 1 for i in range(N))


def test_decrypt_bad_sigma_touches_nothing(engine, sig, batch):
    from drand_amd.engine import SignatureRejected
    _, us, _ = batch
    cs = [message(i, 3) for i in range(2)]
    for bad_cls, s in sorted(T.bad_sigs(sig).items()):
        rc, sc, out, ok, cls = raw_decrypt(engine, s, us[:2], cs, 3)
        assert rc == _lib.BLSV_EINVAL and sc == bad_cls
        assert out.bytes() == b"\xaa" * 6 and ok.bytes() == b"\xaa\xaa" and cls.bytes() == b"\xaa\xaa"
        with pytest.raises(SignatureRejected) as ei:
            engine.tlock_decrypt(s, us[:2], cs)
        assert ei.value.sig_class == bad_cls


@pytest.mark.parametrize("kdf,mlen", [(0, 32), (2, 32), (KDF, 0), (KDF, 257)])
def test_bad_kdf_or_length_is_einval_with_nothing_touched(engine, sig, pk, batch, kdf, mlen):
    rs, us, _ = batch
    width = max(mlen, 1)
    cs = [message(i, width) for i in range(2)]
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, us[:2], cs, mlen, kdf=kdf, out=Guarded(2 * width))
    assert rc == _lib.BLSV_EINVAL and sc == 0xEE
    assert out.bytes() == b"\xaa" * (2 * width) and ok.bytes() == b"\xaa\xaa" and cls.bytes() == b"\xaa\xaa"
    for rounds in (None, [ROUND, ROUND + 1]):
        rc, u, out, ok = raw_encrypt(engine, pk, rs[:2], cs, mlen, kdf=kdf, out=Guarded(2 * width), rounds=rounds)
        assert rc == _lib.BLSV_EINVAL
        assert u.bytes() == b"\xaa" * 96 and out.bytes() == b"\xaa" * (2 * width) and ok.bytes() == b"\xaa\xaa"
    out, ok, cls, sc = Guarded(2 * width), Guarded(2), Guarded(2), Guarded(1)
    rc = engine.lib.blsv_tlock_decrypt_rounds(engine.handle, _lib.buf(sig), (ctypes.c_uint64 * 1)(2), 1,
                                              _lib.buf(us[0] + us[1]), _lib.buf(b"".join(cs)), mlen, 2, kdf, out.ptr, ok.ptr,
                                              cls.ptr, sc.ptr)
    assert rc == _lib.BLSV_EINVAL
    assert out.bytes() == b"\xaa" * (2 * width) and ok.bytes() + cls.bytes() == b"\xaa" * 4 and sc.bytes() == b"\xaa"


@pytest.mark.parametrize("mlen", [3, 32])
def test_in_place(engine, sig, pk, batch, mlen):
    rs, us, gts = batch
    msgs = [message(i, mlen) for i in range(N)]
    cs = masked(gts, msgs)
    buf = Guarded(N * mlen, fill=b"".join(cs))
    rc, sc, out, ok, _ = raw_decrypt(engine, sig, us, buf, mlen, out=buf)
    assert rc == 0 and out is buf and buf.items(mlen) == msgs
    rc, u, out, ok = raw_encrypt(engine, pk, rs, buf, mlen, out=buf)  # the plaintexts are back in buf
    assert rc == 0 and buf.items(mlen) == cs and u.items(48) == us


@pytest.mark.parametrize("mlen,offset", [(32, 0), (3, 1)])
def test_dev_forms(engine, sig, pk, batch, mlen, offset):
    """torch byte tensors: once 4-byte aligned with mlen = 32, once with every pointer offset by one byte
    and mlen = 3; a rejected U among them. All four _dev entry points."""
    import torch
    rs, us, gts = batch
    dev = torch.device("cuda", 0)
    mixed = list(us)
    mixed[5] = T.bad_us()[5]
    msgs = [message(i, mlen) for i in range(N)]
    cs = masked(gts, msgs)

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

    d_us, d_cs = up(b"".join(mixed)), up(b"".join(cs))
    d_out, d_cls = fresh(N * mlen), fresh(N)
    d_out2, d_cls2, d_scls = fresh(N * mlen), fresh(N), fresh(2)
    d_k = up(b"".join(int(k).to_bytes(32, "big") for k in rs))
    d_msgs = up(b"".join(msgs))
    d_u, d_c, d_ok = fresh(N * 48), fresh(N * mlen), fresh(N)
    d_rounds = torch.tensor([ROUND] * N, dtype=torch.int64, device=dev)
    d_u2, d_c2, d_ok2 = fresh(N * 48), fresh(N * mlen), fresh(N)
    torch.cuda.synchronize(dev)  # the fills run on torch's stream, the engine on its own
    p = lambda t: t.data_ptr() + offset
    engine.tlock_decrypt_dev(sig, p(d_us), p(d_cs), mlen, N, p(d_out), p(d_cls))
    engine.tlock_decrypt_rounds_dev([sig, sig], [1, N - 1], p(d_us), p(d_cs), mlen, N, p(d_out2), p(d_cls2), p(d_scls))
    engine.tlock_encrypt_dev(ROUND, p(d_k), p(d_msgs), mlen, N, p(d_u), p(d_c), p(d_ok), pk48=pk)
    engine.tlock_encrypt_rounds_dev(d_rounds.data_ptr(), p(d_k), p(d_msgs), mlen, N, p(d_u2), p(d_c2), p(d_ok2), pk48=pk)
    engine.synchronize()
    torch.cuda.synchronize(dev)
    want = [bytes(mlen) if i == 5 else m for i, m in enumerate(msgs)]
    for o, c in ((d_out, d_cls), (d_out2, d_cls2)):
        assert split(down(o, N * mlen), mlen) == want
        assert down(c, N) == bytes(5 if i == 5 else 0 for i in range(N))
    assert down(d_scls, 2) == bytes(2)
    for u, c, ok in ((d_u, d_c, d_ok), (d_u2, d_c2, d_ok2)):
        assert split(down(u, N * 48), 48) == us and split(down(c, N * mlen), mlen) == cs
        assert down(ok, N) == b"\x01" * N


def test_pass_boundary(engine, sig, pk, batch):
    """n = chunk + 1 with the chunk capped at 16,384: two passes, every item checked. The items are drawn
    cyclically from the 65 known pairs."""
    rs, us, gts = batch
    n, mlen = 16385, 3
    idx = [i % N for i in range(n)]
    msgs = [message(i, mlen) for i in range(n)]
    pads = [callers.kdf_sha256_ctr(g, mlen) for g in gts]
    cs = [xor(m, pads[k]) for m, k in zip(msgs, idx)]
    prev = engine.set_chunk(16384)
    try:
        res = engine.tlock_decrypt(sig, [us[k] for k in idx], cs)
        enc = engine.tlock_encrypt(ROUND, [rs[k] for k in idx], msgs, pk48=pk)
    finally:
        engine.set_chunk(prev)
    assert res.ok == [True] * n and res.msgs == msgs
    assert enc.ok == [True] * n and enc.cs == cs and enc.us == [us[k] for k in idx]


def test_rounds(engine, sigs, sig, batch):
    """Three signatures with counts 0, 1 and 66; then the middle one corrupted."""
    _, us, gts = batch
    mlen = 32
    idx = [i % N for i in range(67)]
    cs = [message(i, mlen) for i in range(67)]
    want = [xor(c, callers.kdf_sha256_ctr(gts[k], mlen)) for c, k in zip(cs, idx)]
    runs = [[], [us[idx[0]]], [us[k] for k in idx[1:]]]
    cruns = [[], cs[:1], cs[1:]]
    before = engine.tlock_open_rounds_stats()[1]
    res = engine.tlock_decrypt_rounds([sigs[8], sig, sig], runs, cruns)
    assert engine.tlock_open_rounds_stats()[1] == before + 67, "counted in the pass it runs"
    assert res.ok == [True] * 67 and res.sig_class == [0, 0, 0] and res.msgs == want
    # distinct signatures: item by item what the opening across rounds gives, then the host KDF
    three = [sigs[8], sigs[9] if 9 in sigs else sigs[8], sig]
    opened = engine.tlock_open_rounds(three, runs)
    assert engine.tlock_decrypt_rounds(three, runs, cruns).msgs == masked(opened.gt, cs)
    assert opened.gt[1:] == [gts[k] for k in idx[1:]] and opened.gt[0] != gts[idx[0]]
    bad_cls, bad = sorted(T.bad_sigs(sig).items())[0]
    res = engine.tlock_decrypt_rounds([sigs[8], bad, sig], runs, cruns)  # returns BLSV_OK: no exception
    assert res.sig_class == [0, bad_cls, 0]
    assert res.ok == [False] + [True] * 66 and res.reject_class == [_lib.REJ_TLOCK_SIG] + [0] * 66
    assert res.msgs == [None] + want[1:]
    # ... and the rejected item's bytes are zeros, not left alone
    out, ok, cls, sc = Guarded(67 * mlen), Guarded(67), Guarded(67), Guarded(3)
    rc = engine.lib.blsv_tlock_decrypt_rounds(engine.handle, _lib.buf(sigs[8] + bad + sig), (ctypes.c_uint64 * 3)(0, 1, 66), 3,
                                              _lib.buf(b"".join(us[k] for k in idx)), _lib.buf(b"".join(cs)), mlen, 67, KDF,
                                              out.ptr, ok.ptr, cls.ptr, sc.ptr)
    assert rc == 0 and out.items(mlen) == [bytes(mlen)] + want[1:] and sc.bytes() == bytes([0, bad_cls, 0])


# ------------------------------------------------------------------ encrypt
@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("mlen", [3, 32, 256])
def test_encrypt_values(engine, pk, batch, n, mlen):
    rs, us, gts = batch
    msgs = [message(i, mlen) for i in range(n)]
    before = engine.tlock_seal_stats()[1]
    rc, u, out, ok = raw_encrypt(engine, pk, rs[:n], msgs, mlen)
    assert rc == 0 and engine.tlock_seal_stats()[1] == before + n, "counted in the pass it runs"
    assert ok.bytes() == b"\x01" * n and u.items(48) == us[:n]
    assert out.items(mlen) == masked(gts[:n], msgs)
    assert u.items(48) == engine.tlock_seal(ROUND, rs[:n], pk48=pk).us


def test_encrypt_is_the_oracle_composition(engine, pk, batch):
    """One item through the support encryptor itself (a pairing of its own)."""
    rs, _, _ = batch
    m = message(2, 100)
    res = engine.tlock_encrypt(ROUND, [rs[20]], [m], pk48=pk)
    assert (res.us[0], res.cs[0]) == T.encrypt(O.g1_decompress(pk), ROUND, m, rs[20], callers.kdf_sha256_ctr)


def test_encrypt_refused_scalar(engine, pk, batch):
    rs, us, gts = batch
    mlen = 3
    ks = list(rs[:5])
    ks[0], ks[3] = 0, O.R
    msgs = [message(i, mlen) for i in range(5)]
    want = masked(gts[:5], msgs)
    for rounds in (None, [ROUND] * 5):
        rc, u, out, ok = raw_encrypt(engine, pk, ks, msgs, mlen, rounds=rounds)
        assert rc == 0 and ok.bytes() == bytes([0, 1, 1, 0, 1])
        assert u.items(48) == [bytes(48) if i in (0, 3) else us[i] for i in range(5)]
        assert out.items(mlen) == [bytes(mlen) if i in (0, 3) else want[i] for i in range(5)]
    res = engine.tlock_encrypt(ROUND, ks, msgs, pk48=pk)
    assert res.ok == [False, True, True, False, True] and res.cs[0] is None and res.us[3] is None


def test_encrypt_rounds(engine, pk, batch):
    """64 distinct rounds: the U bytes and K values are blsv_tlock_seal_rounds's (pinned by its own tests); the
    item locked to ROUND is checked against the oracle."""
    rs, us, gts = batch
    mlen = 33
    rounds = [ROUND + i for i in range(64)]
    msgs = [message(i, mlen) for i in range(64)]
    sealed = engine.tlock_seal_rounds(rounds, rs[:64], pk48=pk)
    before = engine.tlock_seal_rounds_stats()[1]
    res = engine.tlock_encrypt_rounds(rounds, rs[:64], msgs, pk48=pk)
    assert engine.tlock_seal_rounds_stats()[1] == before + 64, "counted in the pass it runs"
    assert res.ok == [True] * 64 and res.us == sealed.us == us[:64]
    assert res.cs == masked(sealed.gt, msgs)
    assert res.cs[0] == xor(msgs[0], callers.kdf_sha256_ctr(gts[0], mlen))
    assert len({g for g in sealed.gt}) == 64


def test_round_trip_under_the_golden_signature(engine, golden, sigs, pk):
    engine.set_public_key(pk)
    msgs = [b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100)), bytes(range(200, 233))]
    cts = callers.timelock_encrypt(engine, ROUND, msgs)  # fresh scalars, the group key
    assert [len(c) for _, c in cts] == [len(m) for m in msgs]
    assert callers.timelock_decrypt(engine, ROUND, sigs[ROUND], cts) == msgs
    assert callers.timelock_open(engine, ROUND, sigs[ROUND], cts, callers.kdf_sha256_ctr) == msgs
    cts_r = callers.timelock_encrypt_rounds(engine, [(ROUND, m) for m in msgs[:2]] + [(ROUND + 1, m) for m in msgs[2:]])
    assert callers.timelock_decrypt_rounds(engine, [(ROUND, sigs[ROUND], cts_r[:2]), (ROUND + 1, sigs[ROUND + 1], cts_r[2:])]) \
        == [msgs[:2], msgs[2:]]
    with pytest.raises(callers.VerifyError):
        callers.timelock_decrypt(engine, ROUND, sigs[ROUND + 1], cts)
    wrong = callers.timelock_decrypt(engine, ROUND, sigs[ROUND + 1], cts, verify=False)
    assert [len(w) for w in wrong] == [len(m) for m in msgs] and wrong[1] != msgs[1] and wrong[2] != msgs[2]


# ------------------------------------------------------------------ the latency path
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("mlen", [3, 32])
def test_latency_path(engine, sig, pk, batch, n, mlen):
    """With both switches at 4, every host form gives the batch path's bytes and the oracle's, counted by the
    latency path's counters alone."""
    rs, us, gts = batch
    pick = [20, 1, 64][:n]  # full-width scalars among them
    u, k, g = [us[i] for i in pick], [rs[i] for i in pick], [gts[i] for i in pick]
    msgs = [message(i, mlen) for i in range(n)]
    cs = masked(g, msgs)
    runs, cruns = [u[:1], u[1:]], [cs[:1], cs[1:]]

    def calls():
        return (engine.tlock_decrypt(sig, u, cs), engine.tlock_decrypt_rounds([sig, sig], runs, cruns),
                engine.tlock_encrypt(ROUND, k, msgs, pk48=pk), engine.tlock_encrypt_rounds([ROUND] * n, k, msgs, pk48=pk))

    def batch_counters():
        return (engine.tlock_stats(), engine.tlock_open_rounds_stats()[1], engine.tlock_seal_stats(),
                engine.tlock_seal_rounds_stats()[1])

    slow = calls()
    prev_o, prev_s = engine.set_tlock_lat_max(4), engine.set_tseal_lat_max(4)
    try:
        counters, lo, ls = batch_counters(), engine.tlock_lat_stats(), engine.tseal_lat_stats()
        fast = calls()
        assert engine.tlock_lat_stats() == (lo[0] + 2, lo[1] + 2 * n), "one launch and n items per call"
        assert engine.tseal_lat_stats() == (ls[0] + 2, ls[1] + 2 * n)
        assert batch_counters() == counters, "the batch counters do not move"
    finally:
        engine.set_tlock_lat_max(0)
        engine.set_tseal_lat_max(0)
    assert (prev_o, prev_s) == (0, 0)
    assert fast == slow
    assert fast[0].msgs == msgs and fast[1].msgs == msgs and fast[1].sig_class == [0, 0]
    assert fast[2].cs == cs and fast[3].cs == cs and fast[2].us == u and fast[3].us == u


def test_latency_path_rejects_and_cutover(engine, sig, pk, batch):
    """A rejected U, a refused scalar and a bad sigma on the latency path; n = 5 takes the batch path."""
    rs, us, gts = batch
    mlen = 3
    msgs = [message(i, mlen) for i in range(5)]
    cs = masked(gts[:5], msgs)
    bad_cls, bad = sorted(T.bad_sigs(sig).items())[0]
    try:
        engine.set_tlock_lat_max(4)
        engine.set_tseal_lat_max(4)
        lo, ls = engine.tlock_lat_stats(), engine.tseal_lat_stats()
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, [us[0], T.bad_us()[5], us[2]], cs[:3], mlen)
        assert rc == 0 and out.items(mlen) == [msgs[0], bytes(mlen), msgs[2]] and cls.bytes() == bytes([0, 5, 0])
        rc, sc, out, ok, cls = raw_decrypt(engine, bad, us[:2], cs[:2], mlen)
        assert rc == _lib.BLSV_EINVAL and sc == bad_cls and out.bytes() == b"\xaa" * 6 and ok.bytes() == b"\xaa\xaa"
        rc, u, out, ok = raw_encrypt(engine, pk, [rs[0], 0, rs[2]], msgs[:3], mlen)
        assert rc == 0 and ok.bytes() == bytes([1, 0, 1])
        assert out.items(mlen) == [cs[0], bytes(mlen), cs[2]] and u.items(48) == [us[0], bytes(48), us[2]]
        assert engine.tlock_lat_stats() == (lo[0] + 2, lo[1] + 5) and engine.tseal_lat_stats() == (ls[0] + 1, ls[1] + 3)
        before = (engine.tlock_stats()[1], engine.tlock_seal_stats()[1])
        assert engine.tlock_decrypt(sig, us[:5], cs).msgs == msgs
        assert engine.tlock_encrypt(ROUND, rs[:5], msgs, pk48=pk).cs == cs
        assert (engine.tlock_stats()[1], engine.tlock_seal_stats()[1]) == (before[0] + 5, before[1] + 5)
        assert engine.tlock_lat_stats() == (lo[0] + 2, lo[1] + 5) and engine.tseal_lat_stats() == (ls[0] + 1, ls[1] + 3)
    finally:
        engine.set_tlock_lat_max(0)
        engine.set_tseal_lat_max(0)
