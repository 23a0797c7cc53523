"""Host-side code under the sanitizers (CPU only; tools/Makefile sanitizer targets).

* the service's request coalescer (drand_amd/csrc/coalesce.h) under ASan+UBSan and under TSan:
  many submitting threads, the dispatcher thread, shutdown while requests are queued;
* the drand.db bulk loader (drand_amd/csrc/boltload.cpp) under ASan+UBSan on bbolt files from
  tests/support/boltwriter.py and 200 truncated / bit-flipped mutants of each (must fail cleanly,
  never fault);
* the engine's device algorithms compiled for the host (tools/opcount.cpp, -DBLS_HOST) under
  ASan+UBSan: field fuzzers and one golden beacon verified end to end.

* the pure logic of the library's HIP-side host units (drand_amd/csrc/hostlogic.h: bitmap packing and
  the class fold, or_bits_at, share selection and index parsing, Fr / Lagrange arithmetic, the
  randomized path's failing-group item count, the service's packed layout) under ASan+UBSan, against
  values computed here in Python.

The GPU-side library cannot run here; what its host units do beyond these parts (the launch sequencing
and copies of blsverify.cpp, verify.cpp, threshold.cpp, tlock.cpp, testhooks.cpp and service.cpp) is
exercised by the GPU suite. DESIGN.md records the one-off run of the whole CPU suite with the ASan
runtime preloaded and the ASan build of libboltload.so.
"""
from __future__ import annotations

import json
import sys
import os
import struct
import subprocess

import pytest

from drand_amd import ingest
from drand_amd.callers import Beacon
from tests.support.boltwriter import write_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")


def _build(target):
    r = subprocess.run(["make", "-C", TOOLS, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(TOOLS, target)


def _run(args, timeout=300):
    r = subprocess.run(args, capture_output=True, text=True, env=SAN_ENV, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("target", ["hosttest-asan", "hosttest-tsan"])
def test_coalescer_sanitized(target):
    out = json.loads(_run([_build(target), "coalesce"]).strip().splitlines()[-1])
    assert out["coalesce"]["items"] > 0


def test_boltload_fuzz_asan(tmp_path, golden):
    ch = golden["chained"]
    bs = [Beacon(bytes.fromhex(b["prev"]), b["round"], bytes.fromhex(b["sig"]), bytes.fromhex(b["sig_v2"]))
          for b in ch["beacons"]]
    items = [(struct.pack(">Q", b.round), ingest.beacon_to_json(b)) for b in bs]
    files = []
    for k, layout in enumerate([dict(per_leaf=5), dict(inline=True), dict(page_size=1024, per_leaf=1)]):
        p = tmp_path / f"f{k}.db"
        write_db(p, items, **layout)
        files.append(str(p))
    out = json.loads(_run([_build("hosttest-asan"), "boltload", *files]).strip().splitlines()[-1])
    assert out["boltload"] == {"files": 3, "mutants": 600}


def test_device_algorithms_on_host_asan(golden):
    exe = _build("opcount-asan")
    assert json.loads(_run([exe, "powfuzz", "200"]))["fp4_sqr_mismatch"] == 0
    assert json.loads(_run([exe, "addfuzz", "100"]))["add_mismatch"] == 0
    out = json.loads(_run([exe, "invfuzz", "500"]))
    assert out["bad"] == 0 and out["unconverged"] == 0
    ch = golden["chained"]
    b = ch["beacons"][1]
    assert json.loads(_run([exe, ch["pk"], str(b["round"]), b["prev"], b["sig"]]))["verified"]
    assert json.loads(_run([exe, ch["pk"], str(b["round"]), "-", b["sig_v2"]]))["verified"]


def test_latency_engine_on_host_asan():
    """tests/test_wv_host.py (the latency engine's lane code compiled for the host, against Python
    integers and the golden fixtures) on the ASan+UBSan build of tools/wvtest."""
    _build("wvtest-asan")
    env = dict(SAN_ENV, WVTEST_TARGET="wvtest-asan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests",
                        "test_wv_host.py")], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]


R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SIZES = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129]


def _bits_to_bytes(bits, nbytes):
    out = bytearray(nbytes)
    for i, b in enumerate(bits):
        if b:
            out[i // 8] |= 1 << (i % 8)
    return bytes(out)


def _select_shares(cls, index, lo, hi, t, n):
    """kyber tbls.Recover's walk: valid shares of [lo, hi) in order until t are held (duplicates count),
    then keyed by index (duplicates collapse) with indices >= n dropped."""
    held = [i for i in range(lo, hi) if cls[i] == 0][:t]
    sel, idx = [], []
    for i in held:
        if index[i] < n and index[i] not in idx:
            sel.append(i)
            idx.append(index[i])
    return {"ok": len(sel) >= t, "sel": sel, "idx": idx}


def test_hostlogic_asan():
    """tools/hosttest.cpp hostlogic: the cases are fixed there and restated here; every expected value
    is computed below (per bit, or with Python integers mod r)."""
    out = json.loads(_run([_build("hosttest-asan"), "hostlogic"]).strip().splitlines()[-1])["hostlogic"]

    # bitmap_words_to_bytes and the latency branch's class fold: one reject at 0, n - 1, the middle, then
    # all three; ceil(n / 8) bytes written, the two 0xEE bytes behind them untouched
    want = []
    for n in SIZES:
        for rej in (0, n - 1, n // 2, n):
            bad = {rej} if rej < n else {0, n - 1, n // 2}
            by = (_bits_to_bytes([i not in bad for i in range(n)], (n + 7) // 8) + b"\xee\xee").hex()
            want.append({"n": n, "bytes": by, "fold": by, "first_bad": min(bad)})
    assert out["verdicts"] == want

    # or_bits_at at every pos % 8: bits [pos, pos + n) of dst get the first n bits of src, the guard byte stays 0
    want = []
    for n in SIZES:
        for s in range(8):
            pos = 8 * (n % 3) + s
            src = bytes((37 * j + 11 * n + 0x5B) & 0xFF for j in range((n + 7) // 8))
            bits = [False] * pos + [bool(src[i // 8] >> (i % 8) & 1) for i in range(n)]
            want.append((_bits_to_bytes(bits, (pos + n + 7) // 8) + b"\x00").hex())
    assert out["or_bits"] == want

    cases = [([0, 0, 0, 0], [3, 3, 5, 6], 0, 4, 3, 10), ([0, 0, 0, 0], [1, 12, 2, 4], 0, 4, 3, 10),
             ([0, 7, 0, 5, 0], [0, 1, 2, 3, 4], 0, 5, 3, 10), ([0, 0, 0], [9, 8, 7], 0, 3, 3, 10),
             ([0, 0], [9, 8], 0, 2, 3, 10), ([0, 0, 0, 0, 0, 6, 0, 0, 0, 0], list(range(10)), 4, 9, 3, 10)]
    want = [_select_shares(*c) for c in cases]
    assert [w["ok"] for w in want] == [False, False, True, True, False, True]  # what each case is there to show
    assert want[0]["idx"] == [3, 5] and want[1]["idx"] == [1, 2] and want[5]["sel"] == [4, 6, 7]
    assert out["select"] == want
    assert out["share_indices"] == [[0, 0x0102, 0xFFFF], [0, 0, 0]]

    # host_lagrange: lambda_i = prod_{j != i} x_j / (x_j - x_i) mod r over x = index + 1
    sets = [[0], [0, 1], [5, 2, 9], [(i * 37 + 11) % 1000 for i in range(33)]]
    assert len(set(sets[3])) == 33
    for idx, got in zip(sets, out["lagrange"]):
        xs = [i + 1 for i in idx]
        for i, xi in enumerate(xs):
            num = den = 1
            for j, xj in enumerate(xs):
                if j != i:
                    num = num * xj % R_ORDER
                    den = den * (xj - xi) % R_ORDER
            assert int(got[i], 16) == num * pow(den, -1, R_ORDER) % R_ORDER
    assert [int(h, 16) for h in out["scalar_mod_r"]] == [v % R_ORDER for v in
                                                         (0, R_ORDER - 1, R_ORDER, R_ORDER + 1, 2 ** 256 - 1)]

    # items in the failing groups of a pass (the short last group included)
    rlc = [(197, 64, [3]), (197, 64, [0, 3]), (128, 64, [1]), (65, 8, [8])]
    assert out["rlc_failing_items"] == [sum(min(cnt, (g + 1) * G) - g * G for g in fail) for cnt, G, fail in rlc]
    assert out["rlc_failing_items"] == [5, 69, 64, 1]

    # the service's packed upload: off[n + 1] | lens[n] | idx[n] | sigs[n][96] | messages, 8-byte aligned parts
    def layout(n, mbytes):
        pad8 = lambda v: (v + 7) // 8 * 8
        o_len = 8 * (n + 1)
        o_idx = o_len + pad8(4 * n)
        o_sig = o_idx + pad8(4 * n)
        o_msg = o_sig + 96 * n
        return [o_len, o_idx, o_sig, o_msg, o_msg + mbytes + 8]
    assert out["svc_layout"] == [layout(*c) for c in [(1, 0), (3, 32), (7, 100), (64, 2048)]]
