"""The pass split rule of the batch pipeline (drand_amd/csrc/hostlogic.h tail_split_main) on the CPU:
tools/tailsplit_test.cpp, a stand-alone program built with ASan+UBSan (tools/Makefile tailsplit-asan)
and run directly, against the rule restated here with Python integers.

main = cnt - cnt % q when q > 0, cnt > q and cnt % q != 0; otherwise cnt (no split).
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
SIZE_MAX = 2 ** 64 - 1
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def rule(cnt, q):
    return cnt - cnt % q if q > 0 and cnt > q and cnt % q else cnt


Q = 65536
CASES = [
    # q = 0: never split
    (0, 0), (1, 0), (1_000_000, 0), (SIZE_MAX, 0),
    # cnt <= q
    (0, Q), (1, Q), (Q - 1, Q), (Q, Q), (5, 4096), (4096, 4096),
    # whole rounds only
    (2 * Q, Q), (15 * Q, Q), (983_040, Q), (1 << 20, Q), (69_632, 4096),
    # one item past a round, and one short of the next
    (Q + 1, Q), (2 * Q - 1, Q), (4097, 4096), (2, 1), (3, 2),
    # the benchmark's pass, the tests' shapes, other round sizes
    (1_000_000, Q), (300_000, Q), (70_003, 4096), (70_003, Q), (70_000, 4096), (1 << 20, 77_824), (300, 128),
    # near SIZE_MAX: no overflow in cnt - cnt % q
    (SIZE_MAX, Q), (SIZE_MAX - 1, Q), (SIZE_MAX, SIZE_MAX), (SIZE_MAX, SIZE_MAX - 1), (SIZE_MAX - 1, SIZE_MAX),
    (SIZE_MAX, 1), (SIZE_MAX, 2), (SIZE_MAX, (1 << 63) + 1), (SIZE_MAX - Q + 1, Q),
]


def test_split_rule_under_sanitizers():
    r = subprocess.run(["make", "-C", TOOLS, "tailsplit-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    args = [str(v) for c in CASES for v in c]
    r = subprocess.run([os.path.join(TOOLS, "tailsplit-asan"), *args], capture_output=True, text=True, env=SAN_ENV,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    got = json.loads(r.stdout)
    assert got == [rule(c, q) for c, q in CASES]
    by = dict(zip(CASES, got))
    # the cases the rule is there for, spelled out
    assert by[(1_000_000, Q)] == 983_040
    assert by[(Q + 1, Q)] == Q and by[(1 << 20, Q)] == 1 << 20 and by[(Q, Q)] == Q and by[(1_000_000, 0)] == 1_000_000
    assert by[(70_003, 4096)] == 69_632 and by[(70_003, Q)] == 65_536
    assert by[(SIZE_MAX, Q)] == SIZE_MAX - (Q - 1) and by[(SIZE_MAX, SIZE_MAX - 1)] == SIZE_MAX - 1
    assert all(m <= c and (m == c or m % q == 0) for (c, q), m in by.items())
