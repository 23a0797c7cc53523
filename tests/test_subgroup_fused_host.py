"""The batch path's subgroup check on the host build (tools/opcount subgroup: drand_amd/csrc/pairing.h
compiled with -DBLS_HOST). The per-item pipeline no longer walks [|x|]sigma in a kernel of its own: the
Miller lines pass walks it anyway, and miller_t_in_subgroup closes psi(sigma) == [x]sigma on the T
that walk leaves. Here that class is compared, point by point, with the class of g2_decompress with
its own psi check (curve.h) and with the Python oracle's decoder. No GPU calls."""
import os
import subprocess

import pytest

from tests.support import subgroup_points as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def _make(target):
    r = subprocess.run(["make", "-C", TOOLS, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(TOOLS, target)


def classes(exe, sigs, env=None):
    """[(batch path's class, g2_decompress(..., true)'s class)] per signature"""
    r = subprocess.run([exe, "subgroup"], input="".join(s.hex() + "\n" for s in sigs), capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode in (0, 1) and not r.stderr, (r.returncode, r.stderr[-4000:])
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(sigs)
    assert (r.returncode == 1) == any(a != b for a, b in rows)
    return rows


@pytest.fixture(scope="module")
def opcount_bin():
    return _make("opcount")


@pytest.fixture(scope="module")
def cases(golden):
    """(name, signature, the Python oracle's class)"""
    out = [("golden chained %d" % b["round"], bytes.fromhex(b["sig"])) for b in golden["chained"]["beacons"]]
    out += [("golden v2 %d" % b["round"], bytes.fromhex(b["sig_v2"])) for b in golden["chained"]["beacons"]]
    out.append(("kat", bytes.fromhex(golden["kat"]["sig"])))
    out += [("mixed %d" % i, bytes.fromhex(s)) for i, s in enumerate(golden["mixed"]["sigs"]) if len(s) == 192]
    out += [("cleared %d" % i, s) for i, s in enumerate(SP.cleared_points(3))]
    out += [("curve %d" % i, s) for i, s in enumerate(SP.random_curve_points(8))]
    out += [("small order %d" % i, s) for i, s in enumerate(SP.all_small_order())]
    out.append(("order 13 r", SP.order_13r_point()))
    out.append(("infinity", bytes([0xC0]) + bytes(95)))
    return [(name, s, SP.oracle_decode_class(s)) for name, s in out]


def test_closing_test_equals_the_psi_check_and_the_oracle(opcount_bin, cases):
    rows = classes(opcount_bin, [s for _, s, _ in cases])
    for (name, _, want), (batch, ref) in zip(cases, rows):
        assert batch == ref == want, (name, batch, ref, want)
    got = [batch for batch, _ in rows]
    names = [name for name, _, _ in cases]
    # the cases cover what they are meant to: accepted points, and every small-order and off-subgroup one rejected
    assert all(got[i] == 0 for i, n in enumerate(names) if n.startswith(("golden", "kat", "cleared", "infinity")))
    assert all(got[i] == 6 for i, n in enumerate(names) if n.startswith(("curve", "small order", "order 13 r")))
    assert sum(n.startswith("small order") for n in names) == 34


def test_closing_test_under_asan_ubsan(cases):
    exe = _make("opcount-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    picked = [c for c in cases if c[0].startswith(("kat", "curve 0", "small order", "order 13 r", "infinity", "mixed"))]
    rows = classes(exe, [s for _, s, _ in picked], env=env)
    assert [batch for batch, _ in rows] == [want for _, _, want in picked]
