"""hostlogic.h tauth_fits / tauth_layout (the guard and the staging layout of blsv_tlock_encrypt_auth* /
blsv_tlock_decrypt_auth*) in tools/hosttest.cpp, a stand-alone program under ASan + UBSan. No GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up8(v):
    return (v + 7) & ~7


def test_guard_and_layout_asan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "hosttest-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "hosttest-asan"), "hostlogic"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["hostlogic"]["tauth"]
    lim = (2 ** 64 - 1) // 1024
    cases = [(1, 1, 0), (1, 256, 1), (1, 32, lim), (1, 32, lim + 1), (1, 0, 1), (1, 257, 1), (0, 32, 1), (2, 32, 1),
             (1, 256, 2 ** 64 - 1), (1, 3, 1 << 20)]
    assert out["fits"] == [kdf == 1 and 1 <= mlen <= 256 and n <= lim for kdf, mlen, n in cases]
    assert out["fits"] == [True, True, True, False, False, False, False, False, False, True]

    def layout(c, mlen):
        secret = up8(64 * c + c * mlen)
        o_out = secret + 8 * c + 48 * c + 32 * c
        o_flag = up8(o_out + c * mlen)
        return [64 * c, secret, o_out, o_flag, o_flag + c]
    assert out["layout"] == [layout(c, m) for c, m in ((1, 1), (64, 3), (65, 33), (16384, 256), (1 << 20, 32))]
