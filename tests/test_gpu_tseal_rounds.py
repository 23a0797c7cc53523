"""Timelock sealing to many rounds on the GPU (blsv_tlock_seal_rounds / _dev, drand_amd/csrc/k_tsealr.hip):
item i sealed to its own round. Against the Python oracle, against the one-round path item by item
(Engine.tlock_seal(round_i, [k_i]), the contract of include/blsverify.h), and through the opening's own
path, blsv_tlock_open(sigma_round_i, U_i) == K_i.

One oracle pairing per distinct round (tests/support/tsealr_ref.py), at most four per test. Shapes: the
one-lane kernels pack 64 items per wave (n = 1, 63, 64, 65), the 3-lane final exponentiation 21 (n = 21,
22, 65); the pass boundary is the context chunk; the rounds differ between neighbouring lanes everywhere,
so a round read from the wrong lane shows.
"""
import ctypes

import pytest

from drand_amd import _lib, callers
from oracle import bls12381 as O
from tests.support import tlock_ref as T
from tests.support import tseal_ref as S
from tests.support import tsealr_ref as SR

pytestmark = pytest.mark.gpu

N = 65


def rounds4(n):
    return [5 + i % 4 for i in range(n)]


@pytest.fixture(scope="module")
def sigs(golden):
    bs = golden["chained"]["beacons"]
    return {b["round"]: bytes.fromhex(b["sig_v2"]) for b in bs if b.get("sig_v2")}


@pytest.fixture(scope="module")
def pk(golden):
    return bytes.fromhex(golden["chained"]["pk"])


@pytest.fixture(scope="module")
def batch(pk):
    """(rounds, scalars, expected (ok, U, K) per item) of the 65-item batch over the four rounds 5..8:
    the module's four oracle pairings, computed once."""
    ks, rs = S.batch65(), rounds4(N)
    want = SR.RoundExpectations(O.g1_decompress(pk))
    return rs, ks, [want(r, k) for r, k in zip(rs, ks)]


@pytest.fixture
def keyed(engine, pk):
    engine.set_public_key(pk)
    return engine


def triples(res):
    return [(ok, u if ok else bytes(48), g if ok else bytes(576)) for ok, u, g in zip(res.ok, res.us, res.gt)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_values(keyed, batch, n):
    rs, ks, want = batch
    res = keyed.tlock_seal_rounds(rs[:n], ks[:n])
    assert triples(res) == want[:n]
    if n == N:
        refused = [i for i, k in enumerate(ks) if k in S.REFUSED]
        assert len(refused) == 3 and [res.ok[i] for i in refused] == [False] * 3
        assert [res.us[i] for i in refused] == [None] * 3 and [res.gt[i] for i in refused] == [None] * 3


def test_equals_the_one_round_path_all_rounds_distinct(keyed):
    """65 distinct rounds, among them 0, 1 and 2^64 - 1: every item is what blsv_tlock_seal gives for its
    round and scalar alone (65 base builds on the existing path)."""
    ks = S.batch65()
    rs = [0, 1, 2 ** 64 - 1] + [(0x9E3779B97F4A7C15 * (i + 1)) % 2 ** 64 for i in range(N - 3)]
    assert len(set(rs)) == N
    res = triples(keyed.tlock_seal_rounds(rs, ks))
    for i, (r, k) in enumerate(zip(rs, ks)):
        assert res[i:i + 1] == triples(keyed.tlock_seal(r, [k])), (i, r)
    assert sum(1 for ok, _, _ in res if not ok) == 3


@pytest.mark.parametrize("n", [21, 22, 65])
def test_round_trip_through_the_opening(keyed, sigs, n):
    """The sealed K of every item equals what the Miller loop and the final exponentiation of the opening
    give for its U under its own round's signature (the golden rounds 1..24)."""
    ks = S.batch65()[:n]
    rs = [1 + i % 24 for i in range(n)]
    res = keyed.tlock_seal_rounds(rs, ks)
    assert res.ok == [k not in S.REFUSED for k in ks]
    for r in sorted(set(rs)):
        mine = [i for i in range(n) if rs[i] == r and res.ok[i]]
        opened = keyed.tlock_open(sigs[r], [res.us[i] for i in mine])
        assert opened.ok == [True] * len(mine)
        assert opened.gt == [res.gt[i] for i in mine], r


def test_pass_boundary(keyed):
    """n = chunk + 65 with the chunk capped at 16,384: two passes, the same bytes as one pass, and both
    the one-round path's over each round's subset."""
    n = 16384 + 65
    ks = list(range(1, n + 1))
    two = (7, 2 ** 63 + 11)
    rs = [two[i % 2] for i in range(n)]
    whole = keyed.tlock_seal_rounds(rs, ks)
    prev = keyed.set_chunk(16384)
    try:
        capped = keyed.tlock_seal_rounds(rs, ks)
    finally:
        keyed.set_chunk(prev)
    assert whole.ok == [True] * n and capped.ok == whole.ok
    assert capped.us == whole.us and capped.gt == whole.gt
    for p, r in enumerate(two):
        sub = keyed.tlock_seal(r, ks[p::2])
        assert sub.us == whole.us[p::2] and sub.gt == whole.gt[p::2], r


def seal_raw(eng, pk48, rounds, ks):
    n = len(ks)
    us = (ctypes.c_uint8 * (48 * n))(*([0xAA] * (48 * n)))
    gt = (ctypes.c_uint8 * (576 * n))(*([0xAA] * (576 * n)))
    ok = (ctypes.c_uint8 * n)(*([0xAA] * n))
    rc = eng.lib.blsv_tlock_seal_rounds(eng.handle, None if pk48 is None else _lib.buf(pk48),
                                        (ctypes.c_uint64 * n)(*rounds), _lib.buf(b"".join(S.be32(k) for k in ks)), n,
                                        us, gt, ok)
    return rc, bytes(us), bytes(gt), bytes(ok)


def test_key_handling(keyed, pk, batch):
    from drand_amd.engine import Engine
    rs, ks, want = batch
    null = keyed.tlock_seal_rounds(rs[:5], ks[:5])
    assert triples(null) == want[:5]
    assert triples(keyed.tlock_seal_rounds(rs[:5], ks[:5], pk48=pk)) == want[:5]
    other_key = O.g1_compress(O.g1_mul(O.G1, 0x1234567))
    res = keyed.tlock_seal_rounds(rs[:5], ks[:5], pk48=other_key)
    assert res.us == null.us and all(a != b for a, b in zip(res.gt, null.gt))
    with Engine(0) as bare:
        rc, us, gt, ok = seal_raw(bare, None, rs[:2], ks[:2])
        assert rc == _lib.BLSV_ENOGROUP
        assert (us, gt, ok) == (b"\xaa" * 96, b"\xaa" * 1152, b"\xaa\xaa")
    for bad in list(T.bad_us().values()) + [b"\xc0" + bytes(47)]:
        rc, us, gt, ok = seal_raw(keyed, bad, rs[:2], ks[:2])
        assert rc == _lib.BLSV_EINVAL, bad.hex()
        assert (us, gt, ok) == (b"\xaa" * 96, b"\xaa" * 1152, b"\xaa\xaa")
    assert triples(keyed.tlock_seal_rounds(rs[:5], ks[:5])) == want[:5]  # the context still seals


def test_cache(pk, sigs, batch):
    """One key-table entry keyed by the key bytes; the one-round base cache, its counters and the
    opening's sigma cache and counters are left alone."""
    from drand_amd.engine import Engine
    rs, ks, want = batch
    other_key = O.g1_compress(O.g1_mul(O.G1, 0x1234567))
    with Engine(0) as eng:
        eng.set_public_key(pk)
        assert eng.tlock_seal_rounds_stats() == (0, 0)
        first = eng.tlock_seal_rounds(rs[:5], ks[:5])
        assert triples(first) == want[:5]
        assert eng.tlock_seal_rounds_stats() == (1, 5)
        assert triples(eng.tlock_seal_rounds(rs[5:16], ks[5:16], pk48=pk)) == want[5:16]  # the same key bytes
        assert eng.tlock_seal_rounds_stats() == (1, 16)  # the refused scalars (11..13) count as items
        eng.tlock_seal_rounds(rs[:2], ks[:2], pk48=other_key)
        assert eng.tlock_seal_rounds_stats() == (2, 18)
        assert triples(eng.tlock_seal_rounds(rs[:2], ks[:2])) == want[:2]
        assert eng.tlock_seal_rounds_stats() == (3, 20)  # A, B, A builds three
        assert eng.tlock_seal_stats() == (0, 0) and eng.tlock_stats() == (0, 0)
        # a call between two one-round seals of one (key, round), and between two openings under one
        # sigma: the base and sigma are each built once
        one = eng.tlock_seal(rs[0], ks[:3])
        a = eng.tlock_open(sigs[1], first.us[:2])
        seal_stats, open_stats = eng.tlock_seal_stats(), eng.tlock_stats()
        assert seal_stats == (1, 3) and open_stats == (1, 2)
        assert triples(eng.tlock_seal_rounds(rs[:5], ks[:5])) == want[:5]
        assert eng.tlock_seal_stats() == seal_stats and eng.tlock_stats() == open_stats
        again = eng.tlock_seal(rs[0], ks[:3])
        b = eng.tlock_open(sigs[1], first.us[:2])
        assert eng.tlock_seal_stats() == (1, 6) and eng.tlock_stats() == (1, 4)
        assert (again.us, again.gt) == (one.us, one.gt) and a.gt == b.gt
        assert triples(one)[0] == want[0]  # item 0 is (rs[0], ks[0]) on both paths


def test_dev_form_equals_host_form(keyed, batch):
    import numpy as np
    import torch
    rs, ks, want = batch
    dev = torch.device("cuda", 0)
    d_rs = torch.from_numpy(np.array(rs, dtype=np.uint64).view(np.int64)).to(dev)
    d_sc = torch.frombuffer(bytearray(b"".join(S.be32(k) for k in ks)), dtype=torch.uint8).to(dev)
    d_us = torch.full((N * 48,), 0xAA, dtype=torch.uint8, device=dev)
    d_gt = torch.full((N * 576,), 0xAA, dtype=torch.uint8, device=dev)
    d_ok = torch.full((N,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)  # the fills run on torch's stream, the engine on its own
    keyed.tlock_seal_rounds_dev(d_rs.data_ptr(), d_sc.data_ptr(), N, d_us.data_ptr(), d_gt.data_ptr(), d_ok.data_ptr())
    keyed.synchronize()
    torch.cuda.synchronize(dev)
    host = keyed.tlock_seal_rounds(rs, ks)
    ub, gb = bytes(d_us.cpu().numpy()), bytes(d_gt.cpu().numpy())
    got = [(bool(o), ub[48 * i:48 * i + 48], gb[576 * i:576 * i + 576]) for i, o in enumerate(d_ok.cpu().numpy())]
    assert got == triples(host)
    assert got == want and sum(1 for ok, _, _ in got if not ok) == 3
    assert bytes(d_sc.cpu().numpy()) == b"".join(S.be32(k) for k in ks)  # the caller's buffers are only read
    assert d_rs.cpu().numpy().view(np.uint64).tolist() == rs


def test_timelock_seal_rounds_end_to_end(keyed, sigs):
    """callers.timelock_seal_rounds on the real engine, every item opened with its own round's signature;
    the next round's signature opens to other bytes of the same lengths."""
    msgs = [b"", b"\x01", bytes(range(32)), bytes((5 * i + 1) % 256 for i in range(100))]
    rounds = [3, 9, 3, 17]
    cts = callers.timelock_seal_rounds(keyed, list(zip(rounds, msgs)), callers.kdf_sha256_ctr)
    assert [len(u) for u, _ in cts] == [48] * 4 and [len(c) for _, c in cts] == [0, 1, 32, 100]
    for r in sorted(set(rounds)):
        mine = [i for i in range(4) if rounds[i] == r]
        got = callers.timelock_open(keyed, r, sigs[r], [cts[i] for i in mine], callers.kdf_sha256_ctr)
        assert got == [msgs[i] for i in mine]
        wrong = callers.timelock_open(keyed, r, sigs[r + 1], [cts[i] for i in mine], callers.kdf_sha256_ctr,
                                      verify=False)
        assert [len(w) for w in wrong] == [len(msgs[i]) for i in mine]
        assert all(w != msgs[i] for w, i in zip(wrong, mine) if len(msgs[i]) >= 32)
