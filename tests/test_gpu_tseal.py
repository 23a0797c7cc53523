"""Timelock sealing on the GPU (blsv_tlock_seal / blsv_tlock_seal_dev, drand_amd/csrc/k_tseal.hip)
against the Python oracle: U_i = k_i G1 and K_i = B^k_i with B = e(pk, H(MessageV2(round)))^3, and
through the opening's own path, blsv_tlock_open(sigma_round, U_i) == K_i.

One oracle pairing per (key, round) (tests/support/tseal_ref.py); every expected value is a power of it.
Shapes: the one-lane kernels pack 64 items per wave (n = 1, 63, 64, 65), the opening's 3-lane final
exponentiation 21 (n = 21, 22, 65); the pass boundary is the context chunk.
"""
import ctypes

import pytest

from drand_amd import _lib, callers
from oracle import bls12381 as O
from tests.support import tlock_ref as T
from tests.support import tseal_ref as S

pytestmark = pytest.mark.gpu

ROUND = 7
N = 65


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def pk(golden):
    return bytes.fromhex(golden["chained"]["pk"])


@pytest.fixture(scope="module")
def kbase(pk):
    return S.kbase(O.g1_decompress(pk), ROUND)  # the module's one pairing for (pk, ROUND)


@pytest.fixture(scope="module")
def batch(kbase):
    """(scalars, expected (ok, U, K) per item) of the 65-item batch, computed once."""
    ks = S.batch65()
    want = S.Expectations(kbase)
    return ks, [want(k) for k in ks]


@pytest.fixture
def keyed(engine, pk):
    engine.set_public_key(pk)
    return engine


def triples(res):
    return [(ok, u if ok else bytes(48), g if ok else bytes(576)) for ok, u, g in zip(res.ok, res.us, res.gt)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_values(keyed, batch, n):
    ks, want = batch
    res = keyed.tlock_seal(ROUND, ks[:n])
    assert triples(res) == want[:n]
    if n == N:
        refused = [i for i, k in enumerate(ks) if k in S.REFUSED]
        assert len(refused) == 3 and [res.ok[i] for i in refused] == [False] * 3
        assert [res.us[i] for i in refused] == [None] * 3


@pytest.mark.parametrize("n", [21, 22, 65])
def test_round_trip_through_the_opening(keyed, sigs, batch, n):
    """The sealed K (table powers in Gt) equals what the Miller loop and the final exponentiation give
    for the sealed U under the round's signature."""
    ks, _ = batch
    res = keyed.tlock_seal(ROUND, ks[:n])
    acc = [i for i in range(n) if res.ok[i]]
    assert len(acc) == n - sum(1 for k in ks[:n] if k in S.REFUSED)
    opened = keyed.tlock_open(sigs[ROUND], [res.us[i] for i in acc])
    assert opened.ok == [True] * len(acc)
    assert opened.gt == [res.gt[i] for i in acc]


def test_pass_boundary(keyed, kbase):
    """n = chunk + 65 with the chunk capped at 16,384: two passes, the same bytes as one pass."""
    n = 16384 + 65
    ks = list(range(1, n + 1))
    whole = keyed.tlock_seal(ROUND, ks)
    prev = keyed.set_chunk(16384)
    try:
        capped = keyed.tlock_seal(ROUND, ks)
    finally:
        keyed.set_chunk(prev)
    assert whole.ok == [True] * n and capped.ok == whole.ok
    assert capped.us == whole.us and capped.gt == whole.gt
    assert whole.us == T.consecutive_us(n)
    assert whole.gt == T.running_gts(kbase, n)


def test_cache(pk, sigs, batch):
    """One base entry keyed by (key bytes, round); the opening's sigma cache survives a seal."""
    from drand_amd.engine import Engine
    ks, want = batch
    with Engine(0) as eng:
        eng.set_public_key(pk)
        assert eng.tlock_seal_stats() == (0, 0)
        first = eng.tlock_seal(ROUND, ks[:3])
        assert triples(first) == want[:3]
        assert eng.tlock_seal_stats() == (1, 3)
        assert triples(eng.tlock_seal(ROUND, ks[3:5])) == want[3:5]
        assert eng.tlock_seal_stats() == (1, 5)
        other = eng.tlock_seal(ROUND + 1, ks[:3])
        assert eng.tlock_seal_stats() == (2, 8)
        assert other.us == first.us and all(a != b for a, b in zip(other.gt, first.gt))
        assert triples(eng.tlock_seal(ROUND, ks[:2])) == want[:2]
        assert eng.tlock_seal_stats() == (3, 10)
        # a seal between two openings under one sigma: sigma is prepared once
        assert eng.tlock_stats() == (0, 0)
        a = eng.tlock_open(sigs[ROUND], first.us)
        eng.tlock_seal(ROUND + 1, ks[:1])
        b = eng.tlock_open(sigs[ROUND], first.us)
        assert eng.tlock_stats() == (1, 6)
        assert a.gt == b.gt == first.gt


def seal_raw(eng, pk48, ks):
    n = len(ks)
    us = (ctypes.c_uint8 * (48 * n))(*([0xAA] * (48 * n)))
    gt = (ctypes.c_uint8 * (576 * n))(*([0xAA] * (576 * n)))
    ok = (ctypes.c_uint8 * n)(*([0xAA] * n))
    rc = eng.lib.blsv_tlock_seal(eng.handle, None if pk48 is None else _lib.buf(pk48), ROUND,
                                 _lib.buf(b"".join(S.be32(k) for k in ks)), n, us, gt, ok)
    return rc, bytes(us), bytes(gt), bytes(ok)


def test_key_handling(keyed, pk, batch):
    from drand_amd.engine import Engine
    ks, want = batch
    null = keyed.tlock_seal(ROUND, ks[:5])
    assert triples(null) == want[:5]
    assert triples(keyed.tlock_seal(ROUND, ks[:5], pk48=pk)) == want[:5]
    other_key = O.g1_compress(O.g1_mul(O.G1, 0x1234567))
    res = keyed.tlock_seal(ROUND, ks[:5], pk48=other_key)
    assert res.us == null.us and all(a != b for a, b in zip(res.gt, null.gt))
    with Engine(0) as bare:
        rc, us, gt, ok = seal_raw(bare, None, ks[:2])
        assert rc == _lib.BLSV_ENOGROUP
        assert (us, gt, ok) == (b"\xaa" * 96, b"\xaa" * 1152, b"\xaa\xaa")
    for bad in list(T.bad_us().values()) + [b"\xc0" + bytes(47)]:
        rc, us, gt, ok = seal_raw(keyed, bad, ks[:2])
        assert rc == _lib.BLSV_EINVAL, bad.hex()
        assert (us, gt, ok) == (b"\xaa" * 96, b"\xaa" * 1152, b"\xaa\xaa")
    assert triples(keyed.tlock_seal(ROUND, ks[:5])) == want[:5]  # the context still seals


def test_dev_form_equals_host_form(keyed, batch):
    import torch
    ks, want = batch
    dev = torch.device("cuda", 0)
    d_sc = torch.frombuffer(bytearray(b"".join(S.be32(k) for k in ks)), dtype=torch.uint8).to(dev)
    d_us = torch.full((N * 48,), 0xAA, dtype=torch.uint8, device=dev)
    d_gt = torch.full((N * 576,), 0xAA, dtype=torch.uint8, device=dev)
    d_ok = torch.full((N,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)  # the fills run on torch's stream, the engine on its own
    keyed.tlock_seal_dev(ROUND, d_sc.data_ptr(), N, d_us.data_ptr(), d_gt.data_ptr(), d_ok.data_ptr())
    keyed.synchronize()
    torch.cuda.synchronize(dev)
    host = keyed.tlock_seal(ROUND, ks)
    ub, gb = bytes(d_us.cpu().numpy()), bytes(d_gt.cpu().numpy())
    got = [(bool(o), ub[48 * i:48 * i + 48], gb[576 * i:576 * i + 576]) for i, o in enumerate(d_ok.cpu().numpy())]
    assert got == triples(host)
    assert got == want and sum(1 for ok, _, _ in got if not ok) == 3


def test_timelock_seal_end_to_end(keyed, sigs):
    """callers.timelock_seal on the real engine, opened with the round's signature; the next round's
    signature opens to other bytes of the same lengths."""
    msgs = [b"", b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100))]
    cts = callers.timelock_seal(keyed, ROUND, msgs, callers.kdf_sha256_ctr)
    assert [len(u) for u, _ in cts] == [48] * 4 and [len(c) for _, c in cts] == [0, 1, 32, 100]
    assert callers.timelock_open(keyed, ROUND, sigs[ROUND], cts, callers.kdf_sha256_ctr) == msgs
    wrong = callers.timelock_open(keyed, ROUND, sigs[ROUND + 1], cts, callers.kdf_sha256_ctr, verify=False)
    assert [len(w) for w in wrong] == [0, 1, 32, 100]
    assert wrong[2] != msgs[2] and wrong[3] != msgs[3]
