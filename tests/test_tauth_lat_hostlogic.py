"""hostlogic.h tauth_lat_routes / tauth_lat_open_layout / tauth_lat_seal_layout (the routing predicate and the
two buffer layouts of the authenticated timelock's latency path, blsv_set_tauth_lat_max) in tools/hosttest.cpp,
a stand-alone program under ASan + UBSan. The layouts are recomputed here in Python. No GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = 2 ** 64 - 1


def up64(v):
    return (v + 63) & ~63


def open_layout(m, n, rounds, idle, mlen):
    o_us = 96 * m
    o_vs = o_us + 48 * n
    o_sigof = o_vs + 32 * n
    o_idle = o_sigof + (4 * n if rounds else 0)
    o_ws = o_idle + 4 * idle
    in_total = o_ws + mlen * n
    o_out = up64(in_total)
    o_cls = o_out + mlen * n
    o_sigcls = o_cls + n
    total = o_sigcls + m
    return [m, n, rounds, idle, mlen, o_us, o_vs, o_sigof, o_idle, o_ws, in_total, o_out, o_cls, o_sigcls, total - o_out, total]


def seal_layout(n, rounds, mlen):
    o_seeds = 8 * n if rounds else 0
    o_msgs = o_seeds + 32 * n
    in_total = o_msgs + mlen * n
    o_us = up64(in_total)
    o_vs = o_us + 48 * n
    o_ws = o_vs + 32 * n
    o_ok = o_ws + mlen * n
    total = o_ok + n
    return [n, rounds, mlen, o_seeds, o_msgs, in_total, o_us, o_vs, o_ws, o_ok, total - o_us, total]


def test_routing_layouts_and_overflow_guard_asan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "hosttest-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "hosttest-asan"), "hostlogic"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["hostlogic"]["tauth_lat"]

    # n = 0, 1, L, L + 1 with L = 4, and L = 0 (the default: nothing routes)
    assert out["routes"] == [[n, lim, 1 <= n <= lim] for n, lim in ((0, 4), (1, 4), (4, 4), (5, 4), (1, 0), (0, 0))]
    assert [r_[2] for r_ in out["routes"]] == [False, True, True, False, False, False]

    # the largest n whose byte counts fit size_t at mlen = 32: per item (or idle signature) at most 186 + 2 mlen
    # bytes when opening, 121 + 2 mlen when sealing, plus at most 63 of padding
    open_most, seal_most = (SIZE_MAX - 63) // (186 + 64), (SIZE_MAX - 63) // (121 + 64)
    assert out["most"] == [open_most, seal_most]
    want_open, want_seal = [], []
    for n, mlen in ((1, 1), (3, 33), (64, 256), (None, 32)):
        for rounds in (0, 1):
            idle = 2 if rounds and n else 0
            k = n if n else open_most
            want_open.append(open_layout(k + idle if rounds else 1, k, rounds, idle, mlen))
            want_seal.append(seal_layout(n if n else seal_most, rounds, mlen))
    assert out["open"] == want_open and out["seal"] == want_seal
    assert all(row[-1] <= SIZE_MAX for row in want_open + want_seal), "the largest n still fits"
    # word arrays are 4-byte aligned, U's words too; the rounds come first in an 8-byte aligned buffer
    assert all(row[7] % 4 == 0 and row[8] % 4 == 0 and row[11] % 64 == 0 for row in want_open)
    assert all(row[6] % 64 == 0 and row[3] % 8 == 0 for row in want_seal)

    # n just above the largest, n + n_idle just above it, a wrapping n + n_idle, more signatures than items and
    # idle signatures together, mlen outside 1 .. 256; then the sealing side's three
    assert out["refused"] == [True] * 8
