"""Signing on the latency path (blsv_set_sign_lat_max, drand_amd/csrc/k_lat_sign.hip: one workgroup of eight
waves per message) on the GPU: against the C oracle, and byte for byte against the batch path (mode off) for
the same arguments -- the signatures, the share-index prefix at stride 98, the infinity encoding of the zero
class, the error codes with untouched outputs -- then the round trip through the verifier, the cutover, the
counters and the setter's contract.

Shapes: one workgroup per message, so n = 1, 2, 9 and 65 (more workgroups than a wave has lanes), with mixed
message lengths around SHA-256's block edges. The keys are chosen by their digits in base |x|
(tests/support/sign_cases.py): each of a workgroup's four ladders runs on one digit.
"""
import ctypes

import pytest

from drand_amd import _lib
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import sign_cases as K

pytestmark = pytest.mark.gpu

BLSV_EINVAL = -1
MAX_CHUNK = 1 << 20  # engine_ctx.h kMaxChunk


def msgs_of(n):
    """n messages of the mixed lengths, each its own bytes"""
    return [K.msg_of(K.MSG_LENS[i % len(K.MSG_LENS)], i) for i in range(n)]


@pytest.fixture(scope="module")
def eng():
    """a context of the module's own: its group and switches are set here"""
    from drand_amd.engine import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def chain_sk(golden):
    return int(golden["chained"]["sk"], 16)


def both_modes(eng, sk, msgs, index=-1):
    """(mode on, mode off) of one sign call, with the counters checked: (1, n) with L on, nothing with L off"""
    n = len(msgs)
    before = eng.sign_lat_stats()
    prev = eng.set_sign_lat_max(128)
    try:
        on = eng.sign(K.be32(sk), msgs, index)
        assert eng.sign_lat_stats() == (before[0] + 1, before[1] + n), "the call took the latency path"
        eng.set_sign_lat_max(0)
        off = eng.sign(K.be32(sk), msgs, index)
        assert eng.sign_lat_stats() == (before[0] + 1, before[1] + n), "with 0 the latency path does not run"
    finally:
        eng.set_sign_lat_max(prev)
    return on, off


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("n", [1, 2, 9, 65])
def test_values(eng, chain_sk, n):
    msgs = msgs_of(n)
    on, off = both_modes(eng, chain_sk, msgs)
    assert len(on) == n and all(len(s) == 96 for s in on)
    for i, m in enumerate(msgs):
        assert on[i] == C.sign(chain_sk, m), (i, len(m))
    assert on == off


@pytest.mark.parametrize("name", list(K.EDGE_KEYS))
def test_edge_keys(eng, name):
    sk = K.EDGE_KEYS[name]
    msgs = [K.MSG32, K.msg_of(55, 1)]
    on, off = both_modes(eng, sk, msgs)
    assert on == [C.sign(sk, m) for m in msgs]
    assert on == off


def test_kat(eng, golden):
    kat = golden["kat"]
    on, off = both_modes(eng, int(kat["sk"], 16), [bytes.fromhex(kat["msg"])])
    assert on == [bytes.fromhex(kat["sig"])] and off == on


# ------------------------------------------------------------------ the share index
COEFFS = [0x1F2E3D4C5B6A79881726354453627180, 0x0123456789ABCDEF0FEDCBA987654321, 0x55AA55AA33CC33CC]  # t = 3


@pytest.mark.parametrize("index", [0, 7, 65535])
def test_share_index(eng, index):
    """BE16(index) || sig at stride 98, equal to mode off; the n = 9 outputs verify as partials of a group
    of n = 4, t = 3 (an index beyond n still has a PubPoly.Eval)."""
    eng.set_group([O.g1_compress(O.g1_mul(O.G1, c)) for c in COEFFS], 4)
    sk = O.pripoly_eval(COEFFS, index)
    for n in (1, 9):
        msgs = msgs_of(n)
        on, off = both_modes(eng, sk, msgs, index)
        assert on == off
        assert all(len(p) == 98 and p[:2] == index.to_bytes(2, "big") for p in on)
        assert [p[2:] for p in on] == [C.sign(sk, m) for m in msgs]
    for m, p in zip(msgs, on):
        ok, cls = eng.verify_partials(m, [p])
        assert ok == [True] and cls == [0], len(m)


# ------------------------------------------------------------------ round trip
def test_round_trip(eng, golden, chain_sk):
    """latency-path signatures of Message and MessageV2 verify under sk_to_pk, and are the chain's own"""
    b = golden["chained"]["beacons"][2]
    msgs = [O.message(b["round"], bytes.fromhex(b["prev"])), O.message_v2(b["round"])]
    on, _ = both_modes(eng, chain_sk, msgs)
    assert [s.hex() for s in on] == [b["sig"], b["sig_v2"]]
    pk = O.g1_compress(O.sk_to_pk(chain_sk))
    assert pk.hex() == golden["chained"]["pk"]
    res = eng.verify_messages(msgs, on, pk48=pk)
    assert res.ok == [True, True]
    assert eng.verify_messages(msgs, on[::-1], pk48=pk).ok == [False, False]


# ------------------------------------------------------------------ the zero class
@pytest.mark.parametrize("name", list(K.ZERO_KEYS))
def test_zero_class(eng, name):
    msgs = msgs_of(3)
    on, off = both_modes(eng, K.ZERO_KEYS[name], msgs)
    assert on == [K.INF_SIG] * 3 and off == on
    on, off = both_modes(eng, K.ZERO_KEYS[name], msgs[:1], 5)
    assert on == [b"\x00\x05" + K.INF_SIG] and off == on


# ------------------------------------------------------------------ errors
def sign_raw(eng, sk32, index, msgs, n, out):
    lens = (ctypes.c_uint32 * max(len(msgs), 1))(*[len(m) for m in msgs])
    return eng.lib.blsv_sign(eng.handle, _lib.buf(sk32), index, _lib.buf(b"".join(msgs)), lens, n, out)


@pytest.mark.parametrize("mode", [128, 0])
def test_errors(eng, chain_sk, mode):
    """a NULL key, index > 65535 and n > kMaxChunk: BLSV_EINVAL before the routing, outputs untouched, no
    counter moved"""
    msgs = msgs_of(2)
    prev = eng.set_sign_lat_max(mode)
    try:
        before = eng.sign_lat_stats()
        for sk32, index, n in ((None, -1, 2), (K.be32(chain_sk), 65536, 2), (K.be32(chain_sk), 3, MAX_CHUNK + 1)):
            out = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
            assert sign_raw(eng, sk32, index, msgs, n, out) == BLSV_EINVAL
            assert bytes(out) == b"\xa5" * 256
        assert eng.sign_lat_stats() == before
        out = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
        assert sign_raw(eng, K.be32(chain_sk), 65535, msgs, 2, out) == 0
        assert bytes(out)[196:] == b"\xa5" * 60 and bytes(out)[:2] == b"\xff\xff"
    finally:
        eng.set_sign_lat_max(prev)


# ------------------------------------------------------------------ cutover, counters, the setter's contract
def other_stats(e):
    return (e.tseal_lat_stats(), e.tlock_lat_stats(), e.tauth_lat_stats(), e.tlock_seal_stats(), e.tlock_stats())


def test_cutover(chain_sk):
    """L = 4: 4 messages take the latency path, 5 the batch path; no other counter moves"""
    from drand_amd.engine import Engine
    msgs = msgs_of(5)
    want = [C.sign(chain_sk, m) for m in msgs]
    with Engine(0) as e:
        others = other_stats(e)
        assert e.set_sign_lat_max(4) == 0
        assert e.sign(K.be32(chain_sk), msgs[:4]) == want[:4]
        assert e.sign_lat_stats() == (1, 4)
        assert e.sign(K.be32(chain_sk), msgs) == want
        assert e.sign_lat_stats() == (1, 4)
        assert e.sign(K.be32(chain_sk), []) == []
        assert e.sign_lat_stats() == (1, 4)
        assert e.sign(K.be32(chain_sk), msgs[4:]) == want[4:]
        assert e.sign_lat_stats() == (2, 5)
        assert other_stats(e) == others


def test_setter_contract(chain_sk):
    from drand_amd.engine import Engine
    with Engine(0) as e:
        assert e.set_sign_lat_max(7) == 0, "the default is 0"
        assert e.set_sign_lat_max(9) == 7, "the previous value comes back"
        assert e.set_tseal_lat_max(0) == 0 and e.set_tlock_lat_max(0) == 0, "the other cutovers are other settings"
        assert e.set_tauth_lat_max() == 0
        lat = e.set_lat_max(5)
        assert e.set_lat_max(lat) == 5
        prev_chunk = e.set_chunk(16384)
        assert e.set_sign_lat_max(10 ** 9) == 9
        assert e.set_sign_lat_max(0) == 16384, "clamped to the chunk"
        e.set_chunk(32768)
        e.set_sign_lat_max(32768)
        assert e.set_tseal_lat_max(0) == 0 and e.set_tlock_lat_max(0) == 0 and e.set_tauth_lat_max() == 0
        e.set_chunk(16384)
        assert e.set_sign_lat_max(0) == 16384, "a shrinking chunk clamps it too"
        e.set_chunk(prev_chunk)
        others = other_stats(e)
        assert e.sign(K.be32(chain_sk), [K.MSG32]) == [C.sign(chain_sk, K.MSG32)]
        assert e.sign_lat_stats() == (0, 0), "with 0 the latency path never runs"
        e.set_sign_lat_max(1)
        assert e.sign(K.be32(chain_sk), [K.MSG32]) == [C.sign(chain_sk, K.MSG32)]
        assert e.sign_lat_stats() == (1, 1) and other_stats(e) == others
        a = ctypes.c_uint64()
        assert e.lib.blsv_sign_lat_stats(e.handle, None, ctypes.byref(a)) == 0 and a.value == 1
        assert e.lib.blsv_sign_lat_stats(e.handle, ctypes.byref(a), None) == 0 and a.value == 1
        assert e.lib.blsv_sign_lat_stats(e.handle, None, None) == 0
