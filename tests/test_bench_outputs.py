"""bench.py --dump-outputs on the CPU: the verdict bitmap's bit order (bit i % 64 of int64 word
i // 64 = round i), the files written for a history WITH rejected rounds, and the seeded sample
taken above DUMP_MAX_ROUNDS rounds. The GPU form (the files a real run writes) is
tests/test_gpu_bench_outputs.py."""
import numpy as np

import bench


def _words(bits):
    w = [0] * ((len(bits) + 63) // 64)
    for i, b in enumerate(bits):
        w[i // 64] |= int(b) << (i % 64)
    return np.array([x - (1 << 64) if x >= 1 << 63 else x for x in w], dtype=np.int64)


def test_unpack_verdicts_bit_order():
    total = 64 * 3 + 5  # whole words and a tail
    bits = np.ones(total, bool)
    bits[[0, 1, 62, 63, 64, 130, 191, 192, total - 1]] = False  # word edges, the sign bit, the last round
    got = bench.unpack_verdicts(_words(bits), total)
    assert got.dtype == bool and got.shape == (total,)
    assert np.flatnonzero(~got).tolist() == [0, 1, 62, 63, 64, 130, 191, 192, total - 1]
    one = bench.unpack_verdicts(np.array([1 << 9], dtype=np.int64), 64)  # a lone accepted round: position 9
    assert np.flatnonzero(one).tolist() == [9]


def test_dump_outputs_writes_the_verdicts_it_is_given(tmp_path):
    ok = np.ones(1000, bool)
    ok[[17, 18, 999]] = False
    bench.dump_outputs(str(tmp_path / "a"), 118, ok)  # first_bad is a ROUND (first_round 101 + index 17)
    got = np.load(tmp_path / "a" / "ok.npy")
    fb = np.load(tmp_path / "a" / "first_bad.npy")
    assert got.dtype == np.float32 and got.shape == (1000,)
    assert np.flatnonzero(got == 0.0).tolist() == [17, 18, 999] and set(got.tolist()) == {0.0, 1.0}
    assert fb.dtype == np.float64 and fb.tolist() == [118.0]
    bench.dump_outputs(str(tmp_path / "b"), None, ok)
    assert np.load(tmp_path / "b" / "first_bad.npy").tolist() == [-1.0]
    # the full-size dump stays under the 64 MB a dump may take
    assert 4 * bench.DUMP_MAX_ROUNDS + 8 + 2 * 128 <= 64 * 1000 * 1000


def test_dump_outputs_samples_large_outputs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ROUNDS", 1000)
    n = 5003
    ok = (np.arange(n) % 7 != 3)  # a pattern that tells positions apart
    bench.dump_outputs(str(tmp_path / "a"), 4, ok)
    bench.dump_outputs(str(tmp_path / "b"), 4, ok)
    a = (tmp_path / "a" / "ok.npy").read_bytes()
    assert a == (tmp_path / "b" / "ok.npy").read_bytes()  # fixed seed: the same sample every time
    got = np.load(tmp_path / "a" / "ok.npy")
    assert got.dtype == np.float32 and got.shape == (1000,)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, 1000))  # the documented recipe
    assert len(set(idx.tolist())) > 800 and idx[0] < n // 10 and idx[-1] > n - n // 10  # spread over the whole output
    assert (got == ok[idx].astype(np.float32)).all()
    ok_at_limit = np.ones(1000, bool)  # exactly DUMP_MAX_ROUNDS rounds: written whole
    ok_at_limit[999] = False
    bench.dump_outputs(str(tmp_path / "c"), 1000, ok_at_limit)
    assert np.flatnonzero(np.load(tmp_path / "c" / "ok.npy") == 0.0).tolist() == [999]
