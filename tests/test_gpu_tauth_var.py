"""The authenticated timelock with a length per item on the GPU (blsv_tlock_encrypt_auth_var, _encrypt_auth_rounds_var,
_decrypt_auth_var, _decrypt_auth_rounds_var; the ragged kernels of drand_amd/csrc/k_tauth.hip and the offset tables
of k_lat_tauth_open.hip / k_lat_tauth_seal.hip).

Expected bytes never come from the code under test: tests/support/tauth_ref.py (hashlib and Python integers) over
ONE oracle pairing for the module, the base of the golden chain's round 7 under its key, and the existing uniform
entry points called once per length. Tampered ciphertexts are ordinary data to every kernel: nothing here provokes
a fault.

Lengths: tauth_ref.MLENS and the edges of the ragged form (the hashed length is 52 + mlen) -- 15, 16, 17 and 79,
80, 81, where 48 + mlen fills a block; 31 .. 33 and 63 .. 65, piece and H4 block edges; 131, 132, 195, 196, where
the padding spills into a second block -- shuffled with a fixed seed, so that neighbouring lanes differ. The 65
items (one wave plus one) cycle through them.

A host form stages its bytes in the engine's own device buffer, whose regions are 8-byte aligned: which store form
a pass runs is decided by its lengths alone (all multiples of 4: dwords), whatever the alignment of the caller's
memory. The misaligned call below therefore pins that the caller's alignment changes no byte.
"""
import ctypes
import random
from contextlib import contextmanager

import numpy as np
import pytest

from drand_amd import _lib
from oracle import bls12381 as O
from tests.support import tauth_ref as A
from tests.support import tlock_ref as T

pytestmark = pytest.mark.gpu

ROUND = 7
N = 65
KDF = _lib.KDF_SHA256_CTR
AUTH = _lib.REJ_TLOCK_AUTH
INF_U = b"\xc0" + bytes(47)
FILL = 0xAA
GUARD = 64

EDGES = [15, 16, 17, 79, 80, 81, 31, 32, 33, 63, 64, 65, 131, 132, 195, 196]
LENS = sorted(set(A.MLENS) | set(EDGES))
random.Random(20240607).shuffle(LENS)
DWORD_LENS = list(A.DWORD_LENS)
random.Random(7).shuffle(DWORD_LENS)


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


def make_items(fb, lens):
    out = []
    for i, mlen in enumerate(lens):
        seed, msg = A.seed_of(3000 + i), A.message(i, mlen)
        k = A.h3(seed, msg)
        v, w = A.seal_tail(seed, msg, T.encode_gt(fb.pow(k)))
        out.append((seed, msg, k, A.u_of(k), v, w))
    assert out[0][3] == T.u_of(out[0][2])
    return tuple(out)


@pytest.fixture(scope="module")
def fb(sig):
    return A.FixedBase(T.gt_base(O.g2_decompress(sig, check_subgroup=False)))


@pytest.fixture(scope="module")
def items(fb):
    """The 65 reference items (seed, msg, k, U, V, W), item i of LENS[i % len(LENS)] bytes: computed once, never
    modified."""
    return make_items(fb, [LENS[i % len(LENS)] for i in range(N)])


@pytest.fixture(scope="module")
def dword_items(fb):
    """65 items whose lengths are all multiples of 4."""
    return make_items(fb, [DWORD_LENS[i % len(DWORD_LENS)] for i in range(N)])


def col(its, k):
    return [it[k] for it in its]


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


def cut(buf, lens):
    out, at = [], 0
    for n in lens:
        out.append(bytes(buf[at:at + n]))
        at += n
    assert at == len(buf)
    return out


class Buf:
    """nbytes (filled with 0xAA or `data`) between two guards of 64 bytes of 0xAA, in numpy memory: 64-byte aligned
    plus `offset`."""

    def __init__(self, nbytes, data=None, offset=0):
        raw = np.full(nbytes + 2 * GUARD + 64 + offset, FILL, dtype=np.uint8)
        start = (-raw.ctypes.data) % 64 + GUARD + offset
        self.raw, self.start, self.n = raw, start, nbytes
        self.view = raw[start:start + nbytes]
        assert (self.view.ctypes.data - offset) % 64 == 0 or nbytes == 0
        if data:
            self.view[:] = np.frombuffer(bytes(data), dtype=np.uint8)
        self.ptr = ctypes.cast(raw.ctypes.data + start, _lib.u8p)

    def bytes(self):
        r = self.raw
        assert (r[:self.start] == FILL).all() and (r[self.start + self.n:] == FILL).all(), "written out of bounds"
        return bytes(self.view)

    def untouched(self):
        return self.bytes() == bytes([FILL]) * self.n


def u32(lens):
    return (ctypes.c_uint32 * max(len(lens), 1))(*lens)


def raw_encrypt(engine, pk, seeds, msgs, lens=None, kdf=KDF, rounds=None, offset=0, in_place=False, n=None):
    """blsv_tlock_encrypt_auth_var (or _rounds_var) over guarded numpy buffers: (rc, us, vs, ws, ok)."""
    lens = [len(m) for m in msgs] if lens is None else lens
    n = len(seeds) if n is None else n
    total = sum(len(m) for m in msgs)
    us, vs, ok = Buf(n * 48, offset=offset), Buf(n * 32, offset=offset), Buf(n, offset=offset)
    min_ = Buf(total, b"".join(msgs), offset=offset)
    ws = min_ if in_place else Buf(total, offset=offset)
    sd = Buf(32 * len(seeds), b"".join(seeds), offset=offset)
    if rounds is None:
        rc = engine.lib.blsv_tlock_encrypt_auth_var(engine.handle, _lib.buf(pk), ROUND, sd.ptr, min_.ptr, u32(lens), n, kdf,
                                                    us.ptr, vs.ptr, ws.ptr, ok.ptr)
    else:
        rc = engine.lib.blsv_tlock_encrypt_auth_rounds_var(engine.handle, _lib.buf(pk), (ctypes.c_uint64 * len(rounds))(*rounds),
                                                           sd.ptr, min_.ptr, u32(lens), n, kdf, us.ptr, vs.ptr, ws.ptr, ok.ptr)
    return rc, us, vs, ws, ok


def raw_decrypt(engine, sig, us, vs, ws, lens=None, kdf=KDF, offset=0, in_place=False, n=None):
    """blsv_tlock_decrypt_auth_var over guarded numpy buffers: (rc, sig_class, out, ok, classes)."""
    lens = [len(w) for w in ws] if lens is None else lens
    n = len(us) if n is None else n
    total = sum(len(w) for w in ws)
    win = Buf(total, b"".join(ws), offset=offset)
    out = win if in_place else Buf(total, offset=offset)
    ok, cls = Buf(n, offset=offset), Buf(n, offset=offset)
    ub, vb = Buf(48 * len(us), b"".join(us), offset=offset), Buf(32 * len(vs), b"".join(vs), offset=offset)
    sc = ctypes.c_uint8(0xEE)
    rc = engine.lib.blsv_tlock_decrypt_auth_var(engine.handle, _lib.buf(sig), ub.ptr, vb.ptr, win.ptr, u32(lens), n, kdf,
                                                out.ptr, ok.ptr, cls.ptr, ctypes.cast(ctypes.byref(sc), _lib.u8p))
    return rc, sc.value, out, ok, cls


@contextmanager
def lat(engine, open_items, seal_items):
    engine.set_tauth_lat_max(open_items, seal_items)
    try:
        yield
    finally:
        engine.set_tauth_lat_max(0, 0)


def batch_counters(engine):
    """(calls or builds, items) of every other path. The key count of the sealing across rounds is left out: the
    latency path builds a key's table through that cache, and the count says so whichever path built it."""
    return (engine.tlock_stats(), engine.tlock_open_rounds_stats(), engine.tlock_seal_stats(),
            (None, engine.tlock_seal_rounds_stats()[1]), engine.tlock_lat_stats(), engine.tseal_lat_stats())


def per_length(its):
    """{length: [indices]} in first-seen order."""
    groups = {}
    for i, it in enumerate(its):
        groups.setdefault(len(it[1]), []).append(i)
    return groups


def uniform_encrypt(engine, pk, its):
    """The existing entry point, one call per distinct length: [(U, V, W)] in item order."""
    out = [None] * len(its)
    for idx in per_length(its).values():
        res = engine.tlock_encrypt_auth(ROUND, [its[i][0] for i in idx], [its[i][1] for i in idx], pk48=pk)
        assert res.ok == [True] * len(idx)
        for i, u, v, w in zip(idx, res.us, res.vs, res.ws):
            out[i] = (u, v, w)
    return out


def check_encrypt(its, us, vs, ws, ok):
    n = len(its)
    assert ok.bytes() == b"\x01" * n
    assert cut(us.bytes(), [48] * n) == col(its, 3) and cut(vs.bytes(), [32] * n) == col(its, 4)
    assert cut(ws.bytes(), [len(it[1]) for it in its]) == col(its, 5)


def check_decrypt(its, out, ok, cls):
    n = len(its)
    assert ok.bytes() == b"\x01" * n and cls.bytes() == bytes(n)
    assert cut(out.bytes(), [len(it[1]) for it in its]) == col(its, 1)


# ------------------------------------------------------------------ 1. one wave plus one, the batch path
def test_one_wave_plus_one_on_the_batch_path(engine, sig, pk, items):
    engine.set_tauth_lat_max(0, 0)
    assert len({len(it[1]) for it in items}) == len(LENS) and all(len(items[i][1]) != len(items[i + 1][1]) for i in range(N - 1))
    c0, l0 = batch_counters(engine), engine.tauth_lat_stats()
    rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1))
    assert rc == 0
    check_encrypt(items, us, vs, ws, ok)
    assert uniform_encrypt(engine, pk, items) == [it[3:6] for it in items]
    res = engine.tlock_encrypt_auth_var(ROUND, col(items, 0), col(items, 1), pk48=pk)
    assert res.ok == [True] * N and (res.us, res.vs, res.ws) == (col(items, 3), col(items, 4), col(items, 5))
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, cut(us.bytes(), [48] * N), cut(vs.bytes(), [32] * N),
                                       cut(ws.bytes(), [len(it[1]) for it in items]))
    assert rc == 0 and sc == 0
    check_decrypt(items, out, ok, cls)
    dec = engine.tlock_decrypt_auth_var(sig, res.us, res.vs, res.ws)
    assert dec.ok == [True] * N and dec.reject_class == [0] * N and dec.msgs == col(items, 1)
    c1 = batch_counters(engine)
    assert engine.tauth_lat_stats() == l0, "the switch is off"
    assert c1[2][1] - c0[2][1] == 3 * N and c1[0][1] - c0[0][1] == 2 * N, "counted in the passes they run"


@pytest.mark.parametrize("offset", [0, 1])
def test_dword_lengths_aligned_and_behind_a_one_byte_offset(engine, sig, pk, dword_items, offset):
    """Every length a multiple of 4: the pass runs the dword form. offset = 0: every buffer of the caller's 64-byte
    aligned; offset = 1: every buffer one byte further. Identical bytes, both equal to the reference."""
    engine.set_tauth_lat_max(0, 0)
    its = dword_items
    assert all(len(it[1]) % 4 == 0 for it in its)
    rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(its, 0), col(its, 1), offset=offset)
    assert rc == 0
    check_encrypt(its, us, vs, ws, ok)
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(its, 3), col(its, 4), col(its, 5), offset=offset)
    assert rc == 0 and sc == 0
    check_decrypt(its, out, ok, cls)
    if offset == 0:
        assert uniform_encrypt(engine, pk, its) == [it[3:6] for it in its]


def test_mixed_lengths_behind_a_one_byte_offset(engine, sig, pk, items):
    engine.set_tauth_lat_max(0, 0)
    rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1), offset=1)
    assert rc == 0
    check_encrypt(items, us, vs, ws, ok)
    rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(items, 3), col(items, 4), col(items, 5), offset=1)
    assert rc == 0 and sc == 0
    check_decrypt(items, out, ok, cls)


# ------------------------------------------------------------------ 2. the latency path
def test_latency_path_same_bytes_one_launch(engine, sig, pk, items):
    c0, l0 = batch_counters(engine), engine.tauth_lat_stats()
    with lat(engine, 128, 128):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(items, 0), col(items, 1))
        rc2, sc, out, ok2, cls = raw_decrypt(engine, sig, col(items, 3), col(items, 4), col(items, 5))
    assert rc == 0 and rc2 == 0 and sc == 0
    check_encrypt(items, us, vs, ws, ok)  # the reference's bytes, which test 1 pins for the batch path
    check_decrypt(items, out, ok2, cls)
    assert engine.tauth_lat_stats() == (l0[0] + 1, l0[1] + N, l0[2] + 1, l0[3] + N), "one launch and 65 items per direction"
    assert batch_counters(engine) == c0, "the batch counters do not move"


@pytest.mark.parametrize("lens", [(1,), (256,), (1, 256), (256, 1)])
def test_latency_path_one_and_two_items(engine, sig, pk, fb, lens):
    its = make_items(fb, list(lens))
    l0 = engine.tauth_lat_stats()
    with lat(engine, 128, 128):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(its, 0), col(its, 1))
        rc2, sc, out, ok2, cls = raw_decrypt(engine, sig, col(its, 3), col(its, 4), col(its, 5))
    assert rc == 0 and rc2 == 0 and sc == 0
    check_encrypt(its, us, vs, ws, ok)
    check_decrypt(its, out, ok2, cls)
    n = len(lens)
    assert engine.tauth_lat_stats() == (l0[0] + 1, l0[1] + n, l0[2] + 1, l0[3] + n)
    rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(its, 0), col(its, 1))  # and the batch path, the same items
    assert rc == 0
    check_encrypt(its, us, vs, ws, ok)


# ------------------------------------------------------------------ 3. rejects keep their place
def tampered(items):
    its = items[:20]
    us, vs, ws = col(its, 3), col(its, 4), col(its, 5)
    ws[3] = flip(ws[3], len(ws[3]) - 1, 0x10)
    vs[7] = flip(vs[7], 13, 0x02)
    us[11] = flip(us[11], 40, 0x01)
    us[15] = INF_U
    u11 = T.g1_class(us[11])  # the reference's decode class of the flipped U; one that decodes fails the check
    want_cls = [AUTH if i in (3, 7, 15) else (u11 or AUTH) if i == 11 else 0 for i in range(20)]
    return its, us, vs, ws, want_cls


@pytest.mark.parametrize("path", ["batch", "latency"])
def test_rejects_keep_their_place(engine, sig, sigs, items, path):
    its, us, vs, ws, want_cls = tampered(items)
    lens = [len(w) for w in ws]
    bad = {3, 7, 11, 15}
    want = [bytes(lens[i]) if i in bad else its[i][1] for i in range(20)]
    with lat(engine, *((128, 128) if path == "latency" else (0, 0))):
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, us, vs, ws)
        assert rc == 0 and sc == 0
        assert list(cls.bytes()) == want_cls and ok.bytes() == bytes(0 if i in bad else 1 for i in range(20))
        assert cut(out.bytes(), lens) == want, "a failing item gets its own length of zeros; every other sits at its offset"
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, us, vs, ws, in_place=True)
        assert rc == 0 and list(cls.bytes()) == want_cls and cut(out.bytes(), lens) == want
        # the wrong round's signature: every item fails the check (item 11 keeps a decode class)
        rc, sc, out, ok, cls = raw_decrypt(engine, sigs[ROUND + 1], us, vs, ws)
        assert rc == 0 and sc == 0 and ok.bytes() == bytes(20) and out.bytes() == bytes(sum(lens))
        assert list(cls.bytes()) == [want_cls[11] if i == 11 else AUTH for i in range(20)]
        # a signature that does not decode: BLSV_EINVAL, the class reported, nothing written
        bad_cls, bad_sig = sorted(T.bad_sigs(sig).items())[0]
        rc, sc, out, ok, cls = raw_decrypt(engine, bad_sig, us, vs, ws)
        assert rc == _lib.BLSV_EINVAL and sc == bad_cls and out.untouched() and ok.untouched() and cls.untouched()
    res = engine.tlock_decrypt_auth_var(sig, us, vs, ws)
    assert res.msgs == [None if i in bad else its[i][1] for i in range(20)] and res.reject_class == want_cls


def test_engine_raises_for_a_signature_that_does_not_decode(engine, sig, items):
    from drand_amd.engine import SignatureRejected
    bad_cls, bad_sig = sorted(T.bad_sigs(sig).items())[0]
    with pytest.raises(SignatureRejected) as ei:
        engine.tlock_decrypt_auth_var(bad_sig, col(items[:3], 3), col(items[:3], 4), col(items[:3], 5))
    assert ei.value.sig_class == bad_cls


# ------------------------------------------------------------------ 4. the rounds forms
@pytest.mark.parametrize("path", ["batch", "latency"])
def test_decrypt_rounds_var(engine, sig, fb, items, path):
    """Four signatures with counts (3, 0, 5, 1), the third undecodable; lengths vary inside each run."""
    its = items[:9]
    bad_cls, bad_sig = sorted(T.bad_sigs(sig).items())[0]
    sg = [sig, sig, bad_sig, sig]
    runs = lambda xs: [xs[:3], [], xs[3:8], xs[8:]]
    us, vs, ws = col(its, 3), col(its, 4), col(its, 5)
    vs[1] = flip(vs[1], 0, 0x80)  # one failing item in a good round
    want_cls = [0, AUTH, 0] + [_lib.REJ_TLOCK_SIG] * 5 + [0]
    want = [m if c == 0 else None for m, c in zip(col(its, 1), want_cls)]
    # the reference agrees on the items that reach the check
    assert A.open_tail(T.encode_gt(fb.pow(its[1][2])), us[1], vs[1], ws[1]) is None
    c0, l0 = batch_counters(engine), engine.tauth_lat_stats()
    with lat(engine, *((128, 128) if path == "latency" else (0, 0))):
        res = engine.tlock_decrypt_auth_rounds_var(sg, runs(us), runs(vs), runs(ws))
        # the raw call: zeros at the failing items' own spans, the guards intact
        lens = [len(w) for w in ws]
        out, ok, cls, sc = Buf(sum(lens)), Buf(9), Buf(9), Buf(4)
        rc = engine.lib.blsv_tlock_decrypt_auth_rounds_var(engine.handle, _lib.buf(b"".join(sg)), (ctypes.c_uint64 * 4)(3, 0, 5, 1),
                                                           4, _lib.buf(b"".join(us)), _lib.buf(b"".join(vs)),
                                                           _lib.buf(b"".join(ws)), u32(lens), 9, KDF, out.ptr, ok.ptr, cls.ptr,
                                                           sc.ptr)
    assert res.sig_class == [0, 0, bad_cls, 0] and res.reject_class == want_cls and res.msgs == want
    assert res.ok == [c == 0 for c in want_cls]
    assert rc == 0 and list(cls.bytes()) == want_cls and list(sc.bytes()) == [0, 0, bad_cls, 0]
    assert cut(out.bytes(), lens) == [m if m is not None else bytes(n) for m, n in zip(want, lens)]
    if path == "latency":
        assert engine.tauth_lat_stats() == (l0[0] + 2, l0[1] + 18, l0[2], l0[3]) and batch_counters(engine) == c0
    else:
        assert engine.tauth_lat_stats() == l0 and batch_counters(engine)[1][1] == c0[1][1] + 18
    # the uniform rounds entry, one call per length: the same classes and messages
    for idx in per_length(its).values():
        pick = lambda xs, lo, hi: [xs[i] for i in idx if lo <= i < hi]
        r = engine.tlock_decrypt_auth_rounds(sg, *[[pick(xs, 0, 3), [], pick(xs, 3, 8), pick(xs, 8, 9)] for xs in (us, vs, ws)])
        assert r.reject_class == [want_cls[i] for i in idx] and r.msgs == [want[i] for i in idx]


@pytest.mark.parametrize("path", ["batch", "latency"])
def test_encrypt_rounds_var_nine_items_to_nine_rounds(engine, sig, pk, items, path):
    """U and K are consistent with blsv_tlock_seal_rounds for the derived scalars (pinned by its own tests); the item
    locked to ROUND is the reference's; every item equals the uniform rounds entry called with its own length."""
    its = items[:9]
    rounds = [ROUND + i for i in range(9)]
    lens = [len(it[1]) for it in its]
    sealed = engine.tlock_seal_rounds(rounds, col(its, 2), pk48=pk)
    with lat(engine, *((128, 128) if path == "latency" else (0, 0))):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(its, 0), col(its, 1), rounds=rounds)
        res = engine.tlock_encrypt_auth_rounds_var(rounds, col(its, 0), col(its, 1), pk48=pk)
    assert rc == 0 and ok.bytes() == b"\x01" * 9 and cut(us.bytes(), [48] * 9) == sealed.us == col(its, 3)
    assert cut(vs.bytes(), [32] * 9) == [A.seal_tail(it[0], it[1], g)[0] for it, g in zip(its, sealed.gt)]
    assert cut(ws.bytes(), lens) == [A.seal_tail(it[0], it[1], g)[1] for it, g in zip(its, sealed.gt)]
    assert (res.us[0], res.vs[0], res.ws[0]) == its[0][3:6] and len(set(sealed.gt)) == 9
    assert (res.us, res.vs, res.ws) == (cut(us.bytes(), [48] * 9), cut(vs.bytes(), [32] * 9), cut(ws.bytes(), lens))
    for i, it in enumerate(its):
        one = engine.tlock_encrypt_auth_rounds([rounds[i]], [it[0]], [it[1]], pk48=pk)
        assert (one.us[0], one.vs[0], one.ws[0]) == (res.us[i], res.vs[i], res.ws[i])
    assert engine.tlock_decrypt_auth_var(sig, res.us[:1], res.vs[:1], res.ws[:1]).msgs == [its[0][1]]


# ------------------------------------------------------------------ 5. the pass boundary
def test_pass_boundary(engine, sig, pk, items):
    """n = 16,384 + 65 under a chunk of 16,384 (two passes, the second sliced at the first's byte count) against the
    same calls under the default chunk (one pass); 32 items, the two on each side of the boundary among them, against
    the reference. The items are drawn cyclically from the 65."""
    engine.set_tauth_lat_max(0, 0)
    n = 16384 + N
    idx = [i % N for i in range(n)]
    seeds, msgs, us, vs, ws = ([items[k][c] for k in idx] for c in (0, 1, 3, 4, 5))
    vs[16383] = flip(vs[16383], 0, 0x80)  # one failing item on each side
    ws[16384] = flip(ws[16384], 0, 0x01)
    cutr = 16000

    def run():
        enc = engine.tlock_encrypt_auth_var(ROUND, seeds, msgs, pk48=pk)
        dec = engine.tlock_decrypt_auth_var(sig, us, vs, ws)
        rdec = engine.tlock_decrypt_auth_rounds_var([sig, sig], [us[:cutr], us[cutr:]], [vs[:cutr], vs[cutr:]],
                                                    [ws[:cutr], ws[cutr:]])
        return enc, dec, rdec
    whole = run()
    prev = engine.set_chunk(16384)
    try:
        split = run()
    finally:
        engine.set_chunk(prev)
    assert split[0] == whole[0] and split[1] == whole[1] and split[2] == whole[2]
    enc, dec, rdec = split
    assert enc.ok == [True] * n and dec.ok == rdec.ok == [i not in (16383, 16384) for i in range(n)]
    assert rdec.sig_class == [0, 0] and rdec.msgs == dec.msgs and rdec.reject_class == dec.reject_class
    sample = sorted({16382, 16383, 16384, 16385, 0, 64, 65, n - 1} | set(random.Random(5).sample(range(n), 24)))
    assert len(sample) == 32
    for i in sample:
        it = items[idx[i]]
        assert (enc.us[i], enc.vs[i], enc.ws[i]) == it[3:6], i
        if i in (16383, 16384):
            assert dec.msgs[i] is None and dec.reject_class[i] == AUTH, i
        else:
            assert dec.msgs[i] == it[1] and dec.reject_class[i] == 0, i


# ------------------------------------------------------------------ 6. the argument rules
@pytest.mark.parametrize("case", ["zero", "long", "kdf", "n0"])
@pytest.mark.parametrize("path", ["batch", "latency"])
def test_argument_rules(engine, sig, pk, items, case, path):
    its = items[:5]
    lens = [len(it[1]) for it in its]
    kdf = 0 if case == "kdf" else KDF
    n = 0 if case == "n0" else 5
    if case == "zero":
        lens[2] = 0
    elif case == "long":
        lens[2] = 257
    want_rc = 0 if case == "n0" else _lib.BLSV_EINVAL
    c0, l0 = batch_counters(engine), engine.tauth_lat_stats()
    with lat(engine, *((128, 128) if path == "latency" else (0, 0))):
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(its, 0), col(its, 1), lens=lens, kdf=kdf, n=n)
        assert rc == want_rc and us.untouched() and vs.untouched() and ws.untouched() and ok.untouched()
        rc, us, vs, ws, ok = raw_encrypt(engine, pk, col(its, 0), col(its, 1), lens=lens, kdf=kdf, n=n,
                                         rounds=[ROUND + i for i in range(5)])
        assert rc == want_rc and us.untouched() and vs.untouched() and ws.untouched() and ok.untouched()
        rc, sc, out, ok, cls = raw_decrypt(engine, sig, col(its, 3), col(its, 4), col(its, 5), lens=lens, kdf=kdf, n=n)
        assert rc == want_rc and sc == (0 if case == "n0" else 0xEE) and out.untouched() and ok.untouched() and cls.untouched()
        out, ok, cls, sc = Buf(sum(len(it[1]) for it in its)), Buf(5), Buf(5), Buf(1)
        rc = engine.lib.blsv_tlock_decrypt_auth_rounds_var(engine.handle, _lib.buf(sig), (ctypes.c_uint64 * 1)(n), 1,
                                                           _lib.buf(b"".join(col(its, 3))), _lib.buf(b"".join(col(its, 4))),
                                                           _lib.buf(b"".join(col(its, 5))), u32(lens), n, kdf, out.ptr, ok.ptr,
                                                           cls.ptr, sc.ptr)
        assert rc == want_rc and out.untouched() and ok.untouched() and cls.untouched()
        assert sc.bytes() == (b"\x00" if case == "n0" else bytes([FILL]))
    assert engine.tauth_lat_stats() == l0
    c1 = batch_counters(engine)
    # items: no counter moves. (n = 0 may prepare a signature or a base, as the uniform forms do: the item counts stay.)
    assert [c[1] for c in c1] == [c[1] for c in c0]
    if case != "n0":
        assert c1 == c0
