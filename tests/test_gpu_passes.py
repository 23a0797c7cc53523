"""The multi-pass loop of the HOST entry points (drand_amd/csrc/verify.cpp run_passes) on the GPU.

The smallest shape that crosses a pass boundary: the smallest chunk (16,384) and n = chunk + 65, with
rejects on both sides of the boundary and in the last item. Expected verdicts follow from the
construction (a valid subgroup point that is the wrong signature fails the pairing check, and in a
chain so does its successor) and are confirmed by the C oracle; every assertion is an exact equality.
The partials case runs one above the latency cutover, where the batch pipeline serves the call.
"""
import hashlib
import os
import random
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
N = CHUNK + 65
FIRST = 5  # first round of the chained range: first_bad is a ROUND, not an index
GEN = 16  # rounds of the fixture chain that the device generator signs again
REJ_PAIRING = 7
PIPELINE = ("hash", "decompress", "miller", "final_exp", "finish")


@pytest.fixture(scope="module")
def C():
    from oracle import c_oracle

    if not os.path.exists(c_oracle.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    c_oracle.load()
    return c_oracle


@pytest.fixture()
def two_passes(engine):
    prev = engine.set_chunk(CHUNK)
    try:
        yield engine
    finally:
        engine.set_chunk(prev)


def message(round_, prev):
    return hashlib.sha256(bytes(prev) + round_.to_bytes(8, "big")).digest()


def rejected(res):
    return [i for i, c in enumerate(res.reject_class) if c]


@pytest.fixture(scope="module")
def chained(engine, golden, C):
    """One continuous chain of N rounds from FIRST under the golden key, rows CHUNK-2, CHUNK and N-1
    replaced by copies of row 7; the oracle's classes at the five rejects and 16 other rows.

    The chain is the committed tests/golden/chain16449_{a,b}.bin (make_chain_fixture.py): a continuous
    chain is sequential to sign, and generate_chained_dev with seg_len = N signs it on ONE lane at 18 ms
    a round (296 s measured on the MI355X for these 16,449). The device generator signs its first GEN
    rounds here, which must be the fixture's."""
    import torch

    ch = golden["chained"]
    pk, seed = bytes.fromhex(ch["pk"]), bytes.fromhex(ch["genesis_seed"])
    engine.set_public_key(pk)
    raw = b""
    for part in ("chain16449_a.bin", "chain16449_b.bin"):
        with open(os.path.join(ROOT, "tests", "golden", part), "rb") as f:
            raw += f.read()
    assert len(raw) == N * 96
    d_seed = torch.zeros(96, dtype=torch.uint8, device="cuda:0")
    d_seed[:32] = torch.tensor(list(seed), dtype=torch.uint8)
    d_sigs = torch.empty(GEN * 96, dtype=torch.uint8, device="cuda:0")
    engine.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), FIRST, GEN, d_seed.data_ptr(), 32,
                                d_sigs.data_ptr(), GEN)
    torch.cuda.synchronize()
    assert bytes(d_sigs.cpu().numpy()) == raw[:GEN * 96]
    sigs = [raw[96 * i:96 * i + 96] for i in range(N)]
    for i in (CHUNK - 2, CHUNK, N - 1):
        sigs[i] = sigs[7]
    bad = [CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, N - 1]
    rng = random.Random(16449)
    others = rng.sample([i for i in range(N) if i not in bad], 16)
    oracle = {i: C.verify(pk, message(FIRST + i, seed if i == 0 else sigs[i - 1]), sigs[i]) for i in bad + others}
    assert all(oracle[i] == REJ_PAIRING for i in bad) and all(oracle[i] == 0 for i in others)
    return {"pk": pk, "seed": seed, "sigs": sigs, "bad": bad, "oracle": oracle}


def check_chained(res, chained):
    cls = [int(c) for c in res.reject_class]
    assert [i for i, c in enumerate(cls) if c] == chained["bad"]
    assert {i: cls[i] for i in chained["oracle"]} == chained["oracle"]
    assert [bool(v) for v in res.ok] == [c == 0 for c in cls]
    assert res.first_bad == FIRST + CHUNK - 2


def test_chained_host_two_passes(two_passes, chained):
    engine = two_passes
    engine.set_public_key(chained["pk"])
    engine.profile(True)
    try:
        engine.profile_read()
        res = engine.verify_chained(FIRST, chained["seed"], chained["sigs"])
        prof = engine.profile_read()
    finally:
        engine.profile(False)
    check_chained(res, chained)
    assert {s: prof[s][1:] for s in PIPELINE} == {s: (2, N) for s in PIPELINE}
    assert prof["lat"][1] == 0 and prof["rlc"][1] == 0


def test_prevs_host_two_passes(two_passes, chained):
    engine = two_passes
    engine.set_public_key(chained["pk"])
    sigs = chained["sigs"]
    prevs = chained["seed"] + bytes(64) + b"".join(sigs[:-1])
    check_chained(engine.verify_prevs(FIRST, 32, prevs, b"".join(sigs), N), chained)


def test_chained_rlc_host_two_passes(two_passes, chained):
    engine = two_passes
    engine.set_public_key(chained["pk"])
    prev_g = engine.set_rlc_group(64)
    engine.test_rlc_seed(bytes(range(32)))
    try:
        s0 = engine.rlc_stats()
        res = engine.verify_chained_rlc(FIRST, chained["seed"], chained["sigs"])
        s1 = engine.rlc_stats()
    finally:
        engine.test_rlc_seed(None)
        engine.set_rlc_group(prev_g)
    check_chained(res, chained)
    # the randomized path served it: 256 + 2 group checks, the groups of the five rejects re-run exactly
    # (CHUNK-2, CHUNK-1 in group 255 of pass 0; CHUNK, CHUNK+1 in group 0 and N-1 alone in group 1 of pass 1)
    assert tuple(b - a for a, b in zip(s0, s1)) == (CHUNK // 64 + 2, 3, 64 + 64 + 1)


@pytest.fixture(scope="module")
def unchained(engine, golden):
    """N V2 signatures (engine.sign over sha256(BE64(round))) for the rounds 1000 + 3 i."""
    ch = golden["chained"]
    rounds = [1000 + 3 * i for i in range(N)]
    msgs = [hashlib.sha256(r.to_bytes(8, "big")).digest() for r in rounds]
    sigs = engine.sign(int(ch["sk"], 16).to_bytes(32, "big"), msgs)
    return {"pk": bytes.fromhex(ch["pk"]), "rounds": rounds, "msgs": msgs, "sigs": sigs}


def test_unchained_host_two_passes(two_passes, unchained, C):
    engine = two_passes
    pk, rounds, msgs = unchained["pk"], unchained["rounds"], unchained["msgs"]
    engine.set_public_key(pk)
    sigs = list(unchained["sigs"])
    bad = [CHUNK - 1, CHUNK]
    for i in bad:
        sigs[i] = unchained["sigs"][7]
    near = [0, CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, N - 1]
    assert [C.verify(pk, msgs[i], sigs[i]) for i in near] == [0, 0, REJ_PAIRING, REJ_PAIRING, 0, 0]
    res = engine.verify_unchained(sigs, rounds=rounds)
    assert rejected(res) == bad and [res.reject_class[i] for i in bad] == [REJ_PAIRING] * 2
    assert res.ok == [i not in bad for i in range(N)]
    assert res.first_bad == rounds[CHUNK - 1]
    prev_g = engine.set_rlc_group(64)
    engine.test_rlc_seed(bytes(range(32)))
    try:
        s0 = engine.rlc_stats()
        got = engine.verify_unchained_rlc(sigs, rounds=rounds)
        s1 = engine.rlc_stats()
    finally:
        engine.test_rlc_seed(None)
        engine.set_rlc_group(prev_g)
    assert (got.ok, got.first_bad, got.reject_class) == (res.ok, res.first_bad, res.reject_class)
    assert s1[0] - s0[0] == CHUNK // 64 + 2 and s1[1] - s0[1] == 2


def test_messages_explicit_pk_two_passes(two_passes, unchained):
    engine = two_passes
    sigs = list(unchained["sigs"])
    bad = [CHUNK - 3, CHUNK + 2]
    for i in bad:
        sigs[i] = unchained["sigs"][7]
    res = engine.verify_messages(unchained["msgs"], sigs, pk48=unchained["pk"])
    assert res.reject_class == [REJ_PAIRING if i in bad else 0 for i in range(N)]
    assert res.ok == [i not in bad for i in range(N)]
    assert res.first_bad == CHUNK - 3


def test_partials_above_the_cutover(engine, golden, C):
    """1,537 partials of one message take the batch pipeline (one pass, hash beside decompression):
    the same verdicts as the latency path, and one profiled hash launch of 1,537 items."""
    th = golden["threshold"]
    commits = [bytes.fromhex(c) for c in th["commits"]]
    msg = bytes.fromhex(th["msg"])
    parts = [bytes.fromhex(p) for p in th["partials"]]
    k = 1537
    batch = [parts[i % len(parts)] for i in range(k)]
    hit = 1000
    batch[hit] = batch[hit][:50] + bytes([batch[hit][50] ^ 4]) + batch[hit][51:]
    engine.set_group(commits, th["n"])
    engine.profile(True)
    try:
        engine.profile_read()
        ok, cls = engine.verify_partials(msg, batch)
        prof = engine.profile_read()
    finally:
        engine.profile(False)
    assert prof["hash"][1:] == (1, k) and prof["lat"][1] == 0
    assert {s: prof[s][1:] for s in PIPELINE} == {s: (1, k) for s in PIPELINE}
    prev = engine.set_lat_max(2048)
    try:
        engine.profile(True)
        engine.profile_read()
        ok_lat, cls_lat = engine.verify_partials(msg, batch)
        prof = engine.profile_read()
    finally:
        engine.profile(False)
        engine.set_lat_max(prev)
    assert prof["lat"][1:] == (1, k) and prof["hash"][1] == 0
    assert (ok, cls) == (ok_lat, cls_lat)
    assert [i for i, c in enumerate(cls) if c] == [hit] and ok == [c == 0 for c in cls]
    grp = C.Group(commits)
    for i in [hit, 0, 63, 64, 999, 1001, 1535, 1536, 777]:
        assert cls[i] == grp.verify_partial(msg, batch[i])
