"""Opt-in randomized batch verification (blsv_verify_*_rlc, drand_amd/csrc/rlc.h, k_rlc.hip) on the GPU.

References: the exact entry points of the same engine (every output of the randomized path must equal
theirs), the C oracle at every corrupted round and its successor, and the Python oracle for the
combination stage's sums. Every assertion is an exact equality.
"""
import hashlib
import os
import subprocess
from contextlib import contextmanager

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (1 << 64) - 1
SEED_A = bytes(range(32))
SEED_B = hashlib.sha256(b"rlc test seed b").digest()
SHAPES = [(8, 43), (64, 337), (None, None)]  # (G, n); None: the default G and n = 4 G + 129


@pytest.fixture(scope="module")
def C():
    from oracle import c_oracle

    if not os.path.exists(c_oracle.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    c_oracle.load()
    return c_oracle


@contextmanager
def rlc_config(engine, group=None, lat_max=0, seed=None):
    """The shared engine with the latency cutover, the group size and the seed set, restored after."""
    prev_lat = engine.set_lat_max(lat_max) if lat_max is not None else None
    prev_g = engine.set_rlc_group(group) if group is not None else None
    engine.test_rlc_seed(seed)
    try:
        g = engine.set_rlc_group(0)  # read the value in force (0 clamps to 8; put it back at once)
        engine.set_rlc_group(g)
        yield g
    finally:
        engine.test_rlc_seed(None)
        if prev_g is not None:
            engine.set_rlc_group(prev_g)
        if prev_lat is not None:
            engine.set_lat_max(prev_lat)


_chain = {"sigs": [], "cls": []}


def chain(engine, golden, n, C=None):
    """(pk, genesis seed, [sigs]) of one continuous n-round chain from round 1: a prefix of one chain the C
    oracle signs (and verifies: every round class 0) once per session, extended when a test needs more."""
    ch = golden["chained"]
    pk, seed = bytes.fromhex(ch["pk"]), bytes.fromhex(ch["genesis_seed"])
    sigs = _chain["sigs"]
    if len(sigs) < n:
        from oracle import c_oracle
        have = len(sigs)
        prev = sigs[-1] if sigs else seed
        for i in range(have, n):
            sigs.append(c_oracle.sign(int(ch["sk"], 16), message(i + 1, sigs[-1] if sigs else seed)))
        _chain["cls"] += c_oracle.verify_chained(pk, have + 1, prev, b"".join(sigs[have:]))
    assert _chain["cls"][:n] == [0] * n  # the reference accepts every round
    engine.set_public_key(pk)
    return pk, seed, list(sigs[:n])


def message(round_, prev):
    return hashlib.sha256(bytes(prev) + round_.to_bytes(8, "big")).digest()


def both(engine, seed, sigs):
    """(exact result, randomized result, stats delta) of the chain from round 1; the two must agree."""
    want = engine.verify_chained(1, seed, sigs)
    s0 = engine.rlc_stats()
    got = engine.verify_chained_rlc(1, seed, sigs)
    s1 = engine.rlc_stats()
    assert got.ok == want.ok and got.first_bad == want.first_bad and got.reject_class == want.reject_class
    return want, got, tuple(b - a for a, b in zip(s0, s1))


def oracle_at(C, pk, seed, sigs, idx):
    return [C.verify(pk, message(i + 1, seed if i == 0 else sigs[i - 1]), sigs[i]) for i in idx]


def shape(engine, g, n):
    if g is None:
        with rlc_config(engine) as dflt:
            return dflt, 4 * dflt + 129
    return g, n


# ------------------------------------------------------------------ 1. the sums
def rlc_scalar(seed, i):
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, "big")).digest()[:8], "big")


def oracle_sum(O, pts, rs):
    """sum r_i P_i with the Python oracle's additions: T_b = the sum of the points whose scalar has bit b,
    then Horner over the bits (the same value as adding the g2_mul results, a third of the additions)."""
    acc = None
    for b in range(63, -1, -1):
        acc = O.g2_add(acc, acc)
        t = None
        for p, r in zip(pts, rs):
            if p is not None and (r >> b) & 1:
                t = O.g2_add(t, p)
        acc = O.g2_add(acc, t)
    return acc


@pytest.mark.parametrize("g,n", [(8, 19), (64, 337)])
def test_sums_match_python_oracle(engine, golden, C, g, n):
    from oracle import bls12381 as O

    pk, seed, sigs = chain(engine, golden, n)
    rej, inf = g + 3, 2 * g + 1
    sigs[rej] = bytes(96)                      # decode reject: in neither sum
    sigs[inf] = bytes([0xC0]) + bytes(95)      # the point at infinity: its H still counts
    with rlc_config(engine, g, seed=SEED_A):
        got_a, got_b = engine.test_rlc_sums(1, seed, sigs)
    hs = [O.g2_decompress(C.hash_to_g2(message(i + 1, seed if i == 0 else sigs[i - 1])), check_subgroup=False)
          for i in range(n)]
    ss = [None if i in (rej, inf) else O.g2_decompress(sigs[i], check_subgroup=False) for i in range(n)]
    rs = [rlc_scalar(SEED_A, i) for i in range(n)]
    if n == 19:  # the bit-plane form itself against g2_mul
        direct = None
        for p, r in zip(hs[:5], rs[:5]):
            direct = O.g2_add(direct, O.g2_mul(p, r))
        assert oracle_sum(O, hs[:5], rs[:5]) == direct
    want_a, want_b = [], []
    for lo in range(0, n, g):
        idx = [i for i in range(lo, min(lo + g, n)) if i != rej]
        want_a.append(O.g2_compress(oracle_sum(O, [hs[i] for i in idx], [rs[i] for i in idx])))
        want_b.append(O.g2_compress(oracle_sum(O, [ss[i] for i in idx], [rs[i] for i in idx])))
    assert got_a == want_a
    assert got_b == want_b


# ------------------------------------------------------------------ 2. all valid
@pytest.mark.parametrize("g,n", SHAPES)
def test_all_valid_chained(engine, golden, C, g, n):
    g, n = shape(engine, g, n)
    pk, seed, sigs = chain(engine, golden, n)
    with rlc_config(engine, g):
        want, got, (groups, failed, exact) = both(engine, seed, sigs)
    assert all(got.ok) and got.first_bad is None and not any(got.reject_class)
    assert groups == -(-n // g) and failed == 0 and exact == 0  # not through the fallback


def test_all_valid_unchained(engine, golden, C):
    g, n = 64, 337
    ch = golden["chained"]
    pk = bytes.fromhex(ch["pk"])
    engine.set_public_key(pk)
    sk32 = int(ch["sk"], 16).to_bytes(32, "big")
    first = 1000
    sigs = engine.sign(sk32, [hashlib.sha256((first + i).to_bytes(8, "big")).digest() for i in range(n)])
    for i in (0, 64, n - 1):
        assert C.verify(pk, hashlib.sha256((first + i).to_bytes(8, "big")).digest(), sigs[i]) == 0
    with rlc_config(engine, g):
        want = engine.verify_unchained(sigs, first_round=first)
        s0 = engine.rlc_stats()
        got = engine.verify_unchained_rlc(sigs, first_round=first)
        s1 = engine.rlc_stats()
        assert (got.ok, got.first_bad, got.reject_class) == (want.ok, want.first_bad, want.reject_class)
        assert all(got.ok) and s1[0] - s0[0] == -(-n // g) and s1[1:] == s0[1:]
        bad = list(sigs)
        bad[70] = sigs[71]
        want = engine.verify_unchained(bad, first_round=first)
        got = engine.verify_unchained_rlc(bad, first_round=first)
        assert (got.ok, got.first_bad, got.reject_class) == (want.ok, want.first_bad, want.reject_class)
        assert got.first_bad == first + 70 and got.ok.count(False) == 1


# ------------------------------------------------------------------ 3. every reject, same outputs
def class_samples(golden):
    """one signature of each decode reject class 2..6 from the golden mixed batch"""
    mx = golden["mixed"]
    out = {}
    for s, c in zip(mx["sigs"], mx["expect_class"]):
        if 2 <= c <= 6 and len(s) == 192:
            out.setdefault(c, bytes.fromhex(s))
    assert sorted(out) == [2, 3, 4, 5, 6]
    return out


@pytest.mark.parametrize("g,n", SHAPES)
def test_every_reject_equals_exact(engine, golden, C, g, n):
    g, n = shape(engine, g, n)
    pk, seed, good = chain(engine, golden, n)
    samples = class_samples(golden)
    cases = [(c, g + 1 + c, samples[c]) for c in range(2, 7)]
    cases += [(7, 5, good[7]),              # a plain bad pairing
              (7, g, good[0]),              # the first item of a group
              (7, 2 * g - 1, good[1]),      # the last item of a group: its successor is in the next one
              (7, n - 2, good[2])]          # inside the ragged last group
    with rlc_config(engine, g):
        for cls, i, sig in cases:
            sigs = list(good)
            sigs[i] = sig
            want, got, (groups, failed, exact) = both(engine, seed, sigs)
            around = [i, i + 1] if i + 1 < n else [i]
            assert [got.reject_class[k] for k in around] == oracle_at(C, pk, seed, sigs, around), (cls, i)
            assert got.reject_class[i] == cls and got.first_bad == i + 1, (cls, i)
            assert got.reject_class[i + 1] == 7 and got.ok.count(False) == 2, (cls, i)
            assert 1 <= failed <= 2 and exact <= 2 * g, (cls, i, failed, exact)


# ------------------------------------------------------------------ 4. cancellation
@pytest.mark.parametrize("seed32", [SEED_A, SEED_B], ids=["seed_a", "seed_b"])
def test_cancelling_pair_is_rejected(engine, golden, C, seed32):
    """sigma_i + D and sigma_j - D in one group leave the group's plain sum unchanged: constant weights
    would accept both."""
    from oracle import bls12381 as O

    g, n = 8, 43
    pk, seed, sigs = chain(engine, golden, n)
    i, j = 17, 21  # both in group 2
    pts = {k: O.g2_decompress(sigs[k], check_subgroup=False) for k in (i, j, 30)}
    d = pts[30]
    plain = O.g2_add(pts[i], pts[j])
    sigs[i] = O.g2_compress(O.g2_add(pts[i], d))
    sigs[j] = O.g2_compress(O.g2_add(pts[j], O.ec_neg(O.FP2, d)))
    assert O.g2_add(O.g2_decompress(sigs[i], check_subgroup=False), O.g2_decompress(sigs[j], check_subgroup=False)) == plain
    with rlc_config(engine, g, seed=seed32):
        want, got, (groups, failed, exact) = both(engine, seed, sigs)
    bad = [i, i + 1, j, j + 1]
    assert [k for k in range(n) if not got.ok[k]] == bad
    assert [got.reject_class[k] for k in bad] == [7] * 4 == oracle_at(C, pk, seed, sigs, bad)
    assert failed == 1 and exact == g


# ------------------------------------------------------------------ 5. duplicates and negations
@pytest.mark.parametrize("negate", [False, True])
def test_repeated_and_negated_neighbours(engine, golden, C, negate):
    g, n = 8, 43
    pk, seed, sigs = chain(engine, golden, n)
    for i in (9, 16, 26):  # inside a lane, at the head of one, and a third group
        s = bytearray(sigs[i])
        if negate:
            s[0] ^= 0x20
        sigs[i + 1] = bytes(s)
    with rlc_config(engine, g):
        want, got, _ = both(engine, seed, sigs)
    idx = [10, 11, 17, 18, 27, 28]
    assert [k for k in range(n) if not got.ok[k]] == idx
    assert [got.reject_class[k] for k in idx] == oracle_at(C, pk, seed, sigs, idx)


# ------------------------------------------------------------------ 6. chunk edge, device buffers
def test_chunk_edge_device_history(engine, golden):
    import torch

    chunk, g, seg = 16384, 64, 64
    n = chunk + 197
    ch = golden["chained"]
    engine.set_public_key(bytes.fromhex(ch["pk"]))
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(23)
    seeds = torch.randint(0, 256, (-(-n // seg) * 96,), dtype=torch.uint8, device="cuda:0", generator=gen)
    sigs = torch.empty(n * 96, dtype=torch.uint8, device="cuda:0")
    engine.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), 1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n)
    torch.cuda.synchronize()
    rows = sigs.view(n, 96)
    for i in (chunk - 3, chunk + 5):  # one corrupted round on each side of the pass boundary
        rows[i].copy_(rows[i - 40].clone())

    def run(fn):
        bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda:0")
        fb = torch.empty(1, dtype=torch.int64, device="cuda:0")
        cls = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        fn(1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n, bm.data_ptr(), fb.data_ptr(), cls.data_ptr())
        torch.cuda.synchronize()
        return bm.cpu().tolist(), int(fb.item()) & NONE, cls.cpu().tolist()

    prev_chunk = engine.set_chunk(chunk)
    try:
        with rlc_config(engine, g):
            want = run(engine.verify_chained_dev)
            s0 = engine.rlc_stats()
            got = run(engine.verify_chained_rlc_dev)
            s1 = engine.rlc_stats()
    finally:
        engine.set_chunk(prev_chunk)
    assert got == want
    bad = [k for k, c in enumerate(got[2]) if c]
    assert bad == [chunk - 3, chunk - 2, chunk + 5, chunk + 6] and got[1] == chunk - 3 + 1
    assert s1[0] - s0[0] == chunk // g + -(-197 // g) and s1[1] - s0[1] == 2 and s1[2] - s0[2] == 2 * g


# ------------------------------------------------------------------ 7. routing
def test_small_calls_take_the_exact_entry_point(engine, golden):
    g = 64
    pk, seed, sigs = chain(engine, golden, 337)
    bad = list(sigs[:2 * g - 1])
    bad[50] = sigs[0]
    with rlc_config(engine, g):  # n = 2 G - 1 on the batch pipeline
        want, got, delta = both(engine, seed, bad)
        assert delta == (0, 0, 0) and got.first_bad == 51
    with rlc_config(engine, 8, lat_max=None):  # n <= lat_max at its default
        bad = list(sigs[:200])
        bad[50] = sigs[0]
        want, got, delta = both(engine, seed, bad)
        assert delta == (0, 0, 0) and got.first_bad == 51


# ------------------------------------------------------------------ 8. callers
def test_callers_fast_matches_default(engine, golden):
    from tests.test_rlc_host import callers_outcomes

    with rlc_config(engine, 8):
        want = callers_outcomes(lambda: engine, golden, False)
        s0 = engine.rlc_stats()
        got = callers_outcomes(lambda: engine, golden, True)
        s1 = engine.rlc_stats()
    assert got == want and want[0][0] == "verified" and want[2][:2] == ("VerifyError", 9)
    assert s1[0] > s0[0] and s1[1] > s0[1]  # the walks of 16 rounds ran the randomized path and its fallback
