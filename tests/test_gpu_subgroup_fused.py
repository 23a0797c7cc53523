"""The subgroup check of the batch pipeline, closed in the Miller lines pass (k_miller_lines<true>,
pairing.h miller_t_in_subgroup) instead of a kernel of its own, on the GPU. Every case forces the
batch pipeline (set_lat_max(0)), and every expected class is the C oracle's (oracle/c) for the same
item: signatures outside G2 must come out REJ_NOT_IN_SUBGROUP, with the reject priority, the bitmap and
first_bad as before, through verify_messages, host and device chained histories (one pass, two passes),
verify_partials, and the randomized entry point, whose head keeps the explicit kernels.
"""
import hashlib
import os
import random
import subprocess

import pytest

from tests.support import subgroup_points as SP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (1 << 64) - 1
N_HISTORY, BAD = 200, 77  # rounds 1..200 of the committed chain; round BAD + 1 carries the bad signature


@pytest.fixture(scope="module")
def C():
    from oracle import c_oracle

    if not os.path.exists(c_oracle.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    c_oracle.load()
    return c_oracle


@pytest.fixture()
def batch_path(engine):
    old = engine.set_lat_max(0)
    yield engine
    engine.set_lat_max(old)


@pytest.fixture(scope="module")
def history(golden, C):
    """(pk, genesis seed, sigs, the C oracle's classes): 200 rounds of tests/golden/chain2049.bin with
    round 78's signature replaced by a curve point outside G2"""
    ch = golden["chained"]
    pk, seed = bytes.fromhex(ch["pk"]), bytes.fromhex(ch["genesis_seed"])
    with open(os.path.join(ROOT, "tests", "golden", "chain2049.bin"), "rb") as f:
        raw = f.read(N_HISTORY * 96)
    sigs = [raw[i * 96:(i + 1) * 96] for i in range(N_HISTORY)]
    sigs[BAD] = SP.random_curve_points(8)[0]
    want = C.verify_chained(pk, 1, seed, b"".join(sigs))
    assert want == [0] * BAD + [6, 7] + [0] * (N_HISTORY - BAD - 2)
    return pk, seed, sigs, want


def test_verify_messages_mixed_batch(batch_path, golden, C):
    """130 items: three one-wave workgroups per pair, the last with two lanes"""
    engine = batch_path
    kat = golden["kat"]
    pk, sk = bytes.fromhex(kat["pk"]), int(kat["sk"], 16)
    mx = golden["mixed"]
    off_curve = next(bytes.fromhex(s) for s, c in zip(mx["sigs"], mx["expect_class"]) if c == 5 and len(s) == 192)
    bad = list(SP.all_small_order()) + list(SP.random_curve_points(8)) + list(SP.cleared_points(3))
    bad += [SP.order_13r_point(), off_curve, bytes([0xC0]) + bytes(95)]
    n = 130
    msgs = [b"subgroup fused %d" % i for i in range(n)]
    slots = list(range(n - 1))
    random.Random(3).shuffle(slots)
    where = dict(zip(slots, bad[1:]))
    where[n - 1] = bad[0]  # a small-order point in the ragged last workgroup
    sigs = [where[i] if i in where else C.sign(sk, msgs[i]) for i in range(n)]
    want = [C.verify(pk, m, s) for m, s in zip(msgs, sigs)]
    assert want.count(0) == n - len(bad) and want.count(6) == 34 + 8 + 1 and 5 in want and want.count(7) == 3 + 1
    res = engine.verify_messages(msgs, sigs, pk48=pk)
    assert res.reject_class == want
    assert res.ok == [c == 0 for c in want] and res.first_bad == next(i for i, c in enumerate(want) if c)


def test_chained_history_one_pass(batch_path, history):
    engine = batch_path
    pk, seed, sigs, want = history
    engine.set_public_key(pk)
    res = engine.verify_chained(1, seed, sigs)
    assert res.reject_class == want
    assert res.reject_class[BAD] == 6 and res.reject_class[BAD + 1] == 7
    assert res.ok == [c == 0 for c in want] and res.first_bad == BAD + 1  # a ROUND


def test_chained_history_two_passes(batch_path, golden, C):
    """base != 0. The smallest pass the engine allows is 16,384 items (engine_ctx.h kMinChunk), past the
    committed chain's 2,049 rounds, so the history is a segmented one generated on the device (as in
    tests/test_gpu_rlc.py), with a curve point outside G2 on each side of the pass boundary. The C
    oracle gives the classes of the bad rounds, their successors and sample rounds around them."""
    import torch

    engine = batch_path
    chunk, seg = 16384, 64
    n = chunk + 197
    ch = golden["chained"]
    pk = bytes.fromhex(ch["pk"])
    engine.set_public_key(pk)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(29)
    seeds = torch.randint(0, 256, (-(-n // seg) * 96,), dtype=torch.uint8, device="cuda:0", generator=gen)
    sigs = torch.empty(n * 96, dtype=torch.uint8, device="cuda:0")
    engine.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), 1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n)
    torch.cuda.synchronize()
    rows = sigs.view(n, 96)
    bad = [chunk - 3, chunk + 5]
    for i, pt in zip(bad, SP.random_curve_points(8)[1:3]):
        rows[i].copy_(torch.tensor(list(pt), dtype=torch.uint8))
    h_seeds, h_rows = bytes(seeds.cpu().tolist()), rows.cpu()

    def sig(i):
        return bytes(h_rows[i].tolist())

    def oracle(i):
        s = i // seg
        prev = h_seeds[s * 96:s * 96 + (32 if s == 0 else 96)] if i % seg == 0 else sig(i - 1)
        return C.verify(pk, hashlib.sha256(prev + (1 + i).to_bytes(8, "big")).digest(), sig(i))

    bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda:0")
    fb = torch.empty(1, dtype=torch.int64, device="cuda:0")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    prev_chunk = engine.set_chunk(chunk)
    try:
        engine.verify_chained_dev(1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n, bm.data_ptr(), fb.data_ptr(),
                                  cls.data_ptr())
        torch.cuda.synchronize()
    finally:
        engine.set_chunk(prev_chunk)
    got = cls.cpu().tolist()
    check = sorted({0, 1, seg, chunk - 4, chunk - 1, chunk, chunk + 4, chunk + 7, n - 1} | set(bad) | {i + 1 for i in bad})
    want = {i: oracle(i) for i in check}
    assert [want[i] for i in bad] == [6, 6] and [want[i + 1] for i in bad] == [7, 7]
    assert all(c == 0 for i, c in want.items() if i not in bad and i - 1 not in bad)
    assert {i: got[i] for i in check} == want
    rejected = [i for i, c in enumerate(got) if c]
    assert rejected == [bad[0], bad[0] + 1, bad[1], bad[1] + 1]
    assert int(fb.item()) & NONE == bad[0] + 1  # a ROUND
    words = [w & NONE for w in bm.cpu().tolist()]
    assert [i for i in range(n) if not (words[i >> 6] >> (i & 63)) & 1] == rejected


def test_verify_partials_one_share_outside_g2(batch_path, golden, C):
    engine = batch_path
    th = golden["threshold"]
    commits = [bytes.fromhex(c) for c in th["commits"]]
    engine.set_group(commits, th["n"])
    msg = bytes.fromhex(th["msg"])
    partials = [bytes.fromhex(p) for p in th["partials"]]
    j = len(partials) // 2
    partials[j] = partials[j][:2] + SP.random_curve_points(8)[3]
    grp = C.Group(commits)
    try:
        want = [grp.verify_partial(msg, p) for p in partials]
    finally:
        grp.close()
    assert want[j] == 6 and want.count(0) == len(partials) - 1
    ok, cls = engine.verify_partials(msg, partials)
    assert cls == want and ok == [c == 0 for c in want]


def test_randomized_entry_point_keeps_its_classes(batch_path, history):
    """verify_chained_rlc sums signatures before any Miller loop, so its head still runs the explicit
    subgroup kernels: same classes as the C oracle and as the exact entry point"""
    engine = batch_path
    pk, seed, sigs, want = history
    engine.set_public_key(pk)
    prev_g = engine.set_rlc_group(8)
    try:
        s0 = engine.rlc_stats()
        res = engine.verify_chained_rlc(1, seed, sigs)
        s1 = engine.rlc_stats()
    finally:
        engine.set_rlc_group(prev_g)
    assert s1[0] - s0[0] == N_HISTORY // 8  # it did take the randomized path
    assert res.reject_class == want and res.first_bad == BAD + 1
