"""Timelock opening on the GPU (blsv_tlock_open / blsv_tlock_open_dev, drand_amd/csrc/k_tlock.hip)
against the Python oracle: E_i = e(U_i, sigma)^3 in the 576-byte encoding of include/blsverify.h.

One oracle pairing per signature, G = e(G1, sigma)^3 (tests/support/tlock_ref.py); every expected
value is G^r for U = r * G1 with a known r. Shapes: the 3-lane final exponentiation packs 21 items per
wave (n = 21, 22, 63) and the one-lane kernels 64 (n = 64, 65); the pass boundary is the context chunk.
"""
import ctypes

import pytest

from drand_amd import _lib, callers
from oracle import bls12381 as O
from tests.support import tlock_ref as T

pytestmark = pytest.mark.gpu

N = 65
WIDE = (0, 10, 20, 21, 22, 62, 63, 64)  # the items with full-width scalars


def scalar(i):
    if i in WIDE:
        return (0x6C1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD * (i + 3) + i) % O.R
    return i + 2


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def sig(sigs):
    assert 7 in sigs, "golden.json carries a V2 signature for round 7"
    return sigs[7]


@pytest.fixture(scope="module")
def base(sig):
    return T.gt_base(O.g2_decompress(sig, check_subgroup=False))  # the module's one pairing for `sig`


@pytest.fixture(scope="module")
def batch(base):
    """(us, expected encodings) of the 65-item batch, computed once."""
    rs = [scalar(i) for i in range(N)]
    return [T.u_of(r) for r in rs], [T.encode_gt(T.gt_pow(base, r)) for r in rs]


@pytest.mark.parametrize("n", [1, 21, 22, 63, 64, 65])
def test_values(engine, sig, batch, n):
    us, want = batch
    res = engine.tlock_open(sig, us[:n])
    assert res.ok == [True] * n and res.reject_class == [0] * n
    assert res.gt == want[:n]


def test_golden_chain_signature_generator(engine, sig, base):
    """The golden chain's round-7 SignatureV2 against the generator alone: the oracle pairing itself."""
    res = engine.tlock_open(sig, [T.u_of(1)])
    assert res.gt == [T.encode_gt(base)]


@pytest.mark.parametrize("cls", [2, 3, 4, 5, 6])
def test_reject_classes(engine, sig, batch, cls):
    us, want = batch
    bad = T.bad_us()[cls]
    assert T.g1_class(bad) == cls
    mixed = list(us)
    for pos in (0, N // 2, N - 1):
        mixed[pos] = bad
    n = len(mixed)
    out = _lib.out_buf(n * 576)
    ok, rc_ = _lib.out_buf(n), _lib.out_buf(n)
    sc = ctypes.c_uint8(9)
    rc = engine.lib.blsv_tlock_open(engine.handle, _lib.buf(sig), _lib.buf(b"".join(mixed)), n, out, ok, rc_,
                                    ctypes.cast(ctypes.byref(sc), _lib.u8p))
    assert rc == 0 and sc.value == 0
    ob = bytes(out)
    for i in range(n):
        got = ob[576 * i:576 * i + 576]
        if i in (0, N // 2, N - 1):
            assert (ok[i], rc_[i], got) == (0, cls, bytes(576)), i
        else:
            assert (ok[i], rc_[i]) == (1, 0) and got == want[i], i


def test_infinity(engine, sig, batch):
    us, want = batch
    mixed = [T.u_of(0)] + us[1:22] + [T.u_of(0)]
    res = engine.tlock_open(sig, mixed)
    assert res.ok == [True] * 23 and res.reject_class == [0] * 23
    assert res.gt == [T.GT_ONE] + want[1:22] + [T.GT_ONE]
    res = engine.tlock_open(b"\xc0" + bytes(95), us[:22])
    assert res.ok == [True] * 22 and res.gt == [T.GT_ONE] * 22


def test_bad_sigma(engine, sig, batch):
    from drand_amd.engine import SignatureRejected
    us, _ = batch
    for cls, s in sorted(T.bad_sigs(sig).items()):
        out = (ctypes.c_uint8 * (2 * 576))(*([0xAA] * (2 * 576)))
        ok = (ctypes.c_uint8 * 2)(0xAA, 0xAA)
        rcl = (ctypes.c_uint8 * 2)(0xAA, 0xAA)
        sc = ctypes.c_uint8(0)
        rc = engine.lib.blsv_tlock_open(engine.handle, _lib.buf(s), _lib.buf(us[0] + us[1]), 2, out, ok, rcl,
                                        ctypes.cast(ctypes.byref(sc), _lib.u8p))
        assert rc == _lib.BLSV_EINVAL and sc.value == cls
        assert bytes(out) == b"\xaa" * (2 * 576) and bytes(ok) == b"\xaa\xaa" and bytes(rcl) == b"\xaa\xaa"
        with pytest.raises(SignatureRejected) as ei:
            engine.tlock_open(s, us[:2])
        assert ei.value.sig_class == cls


def test_pass_boundary(engine, sig, base):
    """n = chunk + 65 with the chunk capped at 16,384: two passes, the same bytes as one pass."""
    n = 16384 + 65
    us = T.consecutive_us(n)
    want = T.running_gts(base, n)
    whole = engine.tlock_open(sig, us)
    prev = engine.set_chunk(16384)
    try:
        capped = engine.tlock_open(sig, us)
    finally:
        engine.set_chunk(prev)
    assert whole.ok == [True] * n and capped.ok == whole.ok
    assert capped.gt == whole.gt
    assert whole.gt == want


def test_cache(sig, sigs, batch):
    """One entry: the same sigma again prepares nothing, another replaces it, the first again re-prepares."""
    from drand_amd.engine import Engine
    us, want = batch
    other = sigs[8]
    with Engine(0) as eng:
        assert eng.tlock_stats() == (0, 0)
        assert eng.tlock_open(sig, us[:3]).gt == want[:3]
        assert eng.tlock_open(sig, us[3:5]).gt == want[3:5]
        assert eng.tlock_stats() == (1, 5)
        assert eng.tlock_open(other, us[:1]).gt != want[:1]
        assert eng.tlock_stats() == (2, 6)
        assert eng.tlock_open(sig, us[:2]).gt == want[:2]
        assert eng.tlock_stats() == (3, 8)


def test_dev_form_equals_host_form(engine, sig, batch):
    import torch
    us, want = batch
    mixed = list(us)
    mixed[5] = T.bad_us()[5]
    dev = torch.device("cuda", 0)
    d_us = torch.frombuffer(bytearray(b"".join(mixed)), dtype=torch.uint8).to(dev)
    d_out = torch.full((N * 576,), 0xAA, dtype=torch.uint8, device=dev)
    d_cls = torch.full((N,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)  # the fills run on torch's stream, the engine on its own
    engine.tlock_open_dev(sig, d_us.data_ptr(), N, d_out.data_ptr(), d_cls.data_ptr())
    engine.synchronize()
    torch.cuda.synchronize(dev)
    host = engine.tlock_open(sig, mixed)
    ob = bytes(d_out.cpu().numpy())
    got = [ob[576 * i:576 * i + 576] for i in range(N)]
    assert list(d_cls.cpu().numpy()) == host.reject_class and host.reject_class[5] == 5
    assert got == [g if g is not None else bytes(576) for g in host.gt]
    assert [g for i, g in enumerate(got) if i != 5] == [w for i, w in enumerate(want) if i != 5]


def test_timelock_open_end_to_end(engine, golden, sigs):
    """Ciphertexts from the support encryptor under kdf_sha256_ctr opened on the real engine; a signature
    of the wrong round is refused with verify=True and opens to other bytes with verify=False."""
    ch = golden["chained"]
    pk = bytes.fromhex(ch["pk"])
    pk_pt = O.g1_decompress(pk)
    engine.set_public_key(pk)
    round_ = 7
    msgs = [b"", b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100))]
    kbase = O.f12_pow(O.pairing(pk_pt, O.hash_to_g2(O.message_v2(round_))), 3)  # one pairing for all four
    cts = []
    for k, m in enumerate(msgs):
        r = scalar(k)
        ks = callers.kdf_sha256_ctr(T.encode_gt(T.gt_pow(kbase, r)), len(m))
        cts.append((T.u_of(r), bytes(a ^ b for a, b in zip(m, ks))))
    assert cts[2] == T.encrypt(pk_pt, round_, msgs[2], scalar(2), callers.kdf_sha256_ctr)  # the encryptor itself
    cts.append((T.bad_us()[6], b"locked to nothing"))
    got = callers.timelock_open(engine, round_, sigs[round_], cts, callers.kdf_sha256_ctr)
    assert got == msgs + [None]
    with pytest.raises(callers.VerifyError):
        callers.timelock_open(engine, round_, sigs[8], cts, callers.kdf_sha256_ctr)
    wrong = callers.timelock_open(engine, round_, sigs[8], cts, callers.kdf_sha256_ctr, verify=False)
    assert wrong[4] is None and wrong[0] == b""
    assert wrong[2] != msgs[2] and wrong[3] != msgs[3] and len(wrong[3]) == 100
