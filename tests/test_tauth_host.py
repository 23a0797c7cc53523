"""The authenticated timelock on the host build (tools/opcount tauth: drand_amd/csrc/tauth.h compiled with
-DBLS_HOST, the reduction, the streamed H3, H4, the check and the stores as k_tauth.hip runs them) against
tests/support/tauth_ref.py (hashlib and Python integers), and the callers.timelock_*_auth family on a stand-in
engine backed by the oracle. No GPU.

The tool's tails take K / E as given bytes, so its cases need no pairing: any twelve canonical Fp values serve.
A compact subset runs once more through opcount-asan (a stand-alone program under ASan + UBSan).
"""
import hashlib
import json
import os
import subprocess

import pytest

from drand_amd import callers
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import tauth_ref as A
from tests.support import tlock_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
ROUND = 7


def build(target):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), target], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", target)


@pytest.fixture(scope="module")
def opcount_bin():
    return build("opcount")


@pytest.fixture(scope="module")
def opcount_asan_bin():
    return build("opcount-asan")


def some_gt(tag):
    """576 bytes of twelve canonical Fp values (the tails hash them as they are)."""
    out = b""
    for k in range(12):
        v = int.from_bytes(hashlib.sha512(b"tauth-gt" + bytes([tag, k])).digest(), "big") % O.P
        out += v.to_bytes(48, "big")
    return out


def run_tauth(binp, mlen, lines):
    r = subprocess.run([binp, "tauth"], input="%d\n" % mlen + "".join(l + "\n" for l in lines), capture_output=True,
                       text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


# ------------------------------------------------------------------ the reduction
def reduce_values():
    r = O.R
    top = ((1 << 384) // r) * r
    if top == 1 << 384:
        top -= r
    vals = [0, 1, r - 1, r, r + 1, 2 * r, top, (1 << 256) - 1, 1 << 256, (1 << 384) - 1]
    for i in range(16):
        vals.append(int.from_bytes(hashlib.sha384(b"tauth-reduce" + bytes([i])).digest(), "big"))
    return vals


def check_reduce(binp):
    vals = reduce_values()
    rc, out = run_tauth(binp, 1, ["reduce %s" % v.to_bytes(48, "big").hex() for v in vals])
    assert rc == 0 and len(out["reduce"]) == len(vals)
    for v, got in zip(vals, out["reduce"]):
        assert int(got["k"], 16) == v % O.R, hex(v)
        assert got["nonzero"] is (v % O.R != 0), hex(v)  # 0, r, 2r and the largest multiple are refused
    assert [g["nonzero"] for g in out["reduce"][:7]] == [False, True, True, False, True, False, False]


def test_reduce384_matches_python_integers(opcount_bin):
    check_reduce(opcount_bin)


# ------------------------------------------------------------------ both tails, every length
def seal_cases(mlen, n=3):
    return [(A.seed_of(100 * mlen + i), A.message(i, mlen), some_gt(i)) for i in range(n)]


def check_tails(binp, mlen):
    cases = seal_cases(mlen)
    want = []
    lines = []
    for seed, msg, gt in cases:
        k = A.h3(seed, msg)
        v, w = A.seal_tail(seed, msg, gt)
        want.append((k, v, w))
        lines.append("seal %s %s %s" % (seed.hex(), msg.hex(), gt.hex()))
        lines.append("open %s %s %s %s" % (gt.hex(), T.u_of(k).hex(), v.hex(), w.hex()))
    rc, out = run_tauth(binp, mlen, lines)
    assert rc == 0 and out["forms_match"] is True  # both store forms and the in-place run agree, guards intact
    for (k, v, w), got in zip(want, out["seal"]):
        assert got["ok"] == 1 and int(got["k"], 16) == k
        assert bytes.fromhex(got["v"]) == v and bytes.fromhex(got["w"]) == w
    for (seed, msg, gt), got in zip(cases, out["open"]):
        assert got["cls"] == 0 and bytes.fromhex(got["msg"]) == msg
    assert 0 < out["fp_mul_open"] < 64 * 16 + 16  # at most 64 mixed additions and the comparison


@pytest.mark.parametrize("mlen", A.MLENS)
def test_seal_and_open_tails_match_the_reference(opcount_bin, mlen):
    check_tails(opcount_bin, mlen)


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


def check_verdicts(binp, mlen):
    cts = []
    for seed, msg, gt in seal_cases(mlen, 9):
        k = A.h3(seed, msg)
        v, w = A.seal_tail(seed, msg, gt)
        cts.append([gt, T.u_of(k), v, w, 0, msg, k])
    cts[1][2] = flip(cts[1][2], 17, 0x10)  # a V bit
    cts[2][3] = flip(cts[2][3], 0)  # the first W byte
    cts[3][3] = flip(cts[3][3], mlen - 1, 0x80)  # the last W byte
    cts[4][1] = T.u_of(cts[4][6] + 1)  # U = (k + 1) G1
    cts[5][1] = T.u_of(0)  # U at infinity
    cts[6][0] = T.GT_ONE  # E = 1
    cts[7][4] = 5  # arrives with a decode class
    bad = {1, 2, 3, 4, 5, 6, 7}
    rc, out = run_tauth(binp, mlen, ["open %s %s %s %s %d" % (g.hex(), u.hex(), v.hex(), w.hex(), c)
                                     for g, u, v, w, c, _, _ in cts])
    assert rc == 0 and out["forms_match"] is True
    for i, (ct, got) in enumerate(zip(cts, out["open"])):
        if i in bad:
            assert got["cls"] == (5 if i == 7 else A.REJ_TLOCK_AUTH), i
            assert bytes.fromhex(got["msg"]) == bytes(mlen), i
        else:
            assert got["cls"] == 0 and bytes.fromhex(got["msg"]) == ct[5], i
    # the reference agrees on every item that reaches the check
    for i, (g, u, v, w, c, msg, _) in enumerate(cts):
        if i != 7:
            assert A.open_tail(g, u, v, w) == (None if i in bad else msg), i


@pytest.mark.parametrize("mlen", [3, 32, 76])
def test_open_verdicts(opcount_bin, mlen):
    check_verdicts(opcount_bin, mlen)


def test_an_undecodable_u_keeps_its_class(opcount_bin):
    seed, msg, gt = seal_cases(4, 1)[0]
    v, w = A.seal_tail(seed, msg, gt)
    bad = T.bad_us()
    rc, out = run_tauth(opcount_bin, 4, ["open %s %s %s %s" % (gt.hex(), bad[c].hex(), v.hex(), w.hex()) for c in sorted(bad)])
    assert rc == 0 and [g["cls"] for g in out["open"]] == sorted(bad)
    assert all(bytes.fromhex(g["msg"]) == bytes(4) for g in out["open"])


def test_the_same_cases_under_asan(opcount_asan_bin):
    check_reduce(opcount_asan_bin)
    for mlen in (1, 3, 12, 33, 256):
        check_tails(opcount_asan_bin, mlen)
    check_verdicts(opcount_asan_bin, 3)
    check_verdicts(opcount_asan_bin, 32)


def test_tool_refuses_lengths_outside_the_cap(opcount_bin):
    for mlen in (0, 257):
        r = subprocess.run([opcount_bin, "tauth"], input="%d\n" % mlen, capture_output=True, text=True)
        assert r.returncode == 2 and not r.stdout


# ------------------------------------------------------------------ the callers, stand-in engine
class AuthStandIn(T.OracleTlockEngine):
    """The oracle stand-in with the authenticated Engine methods, answered by tauth_ref: every U it opens is one it
    sealed (k looked up by U), under one pairing per distinct signature."""

    def verify_unchained(self, sigs, first_round=None, rounds=None):
        from drand_amd.engine import BatchResult
        self.calls.append("verify_unchained")
        if rounds is None:
            rounds = [first_round + i for i in range(len(sigs))]
        cls = [self.c.verify(self.pk, O.message_v2(r), bytes(s)) for r, s in zip(rounds, sigs)]
        bad = [i for i, c in enumerate(cls) if c]
        return BatchResult([c == 0 for c in cls], bad[0] if bad else None, cls)

    @staticmethod
    def _one_length(items):
        lens = {len(x) for x in items}
        assert len(lens) == 1 and 1 <= min(lens) <= 256, "the engine takes one length 1 .. 256 per call"

    def _base(self, round_):
        key = ("round", round_)
        if key not in self.bases:
            self.bases[key] = O.f12_pow(O.pairing(O.g1_decompress(self.pk), O.hash_to_g2(O.message_v2(round_))), 3)
        return self.bases[key]

    def tlock_encrypt_auth(self, round_, seeds, msgs, pk48=None, kdf=1):
        return self.tlock_encrypt_auth_rounds([round_] * len(msgs), seeds, msgs, pk48, kdf, name="tlock_encrypt_auth")

    def tlock_encrypt_auth_rounds(self, rounds, seeds, msgs, pk48=None, kdf=1, name="tlock_encrypt_auth_rounds"):
        from drand_amd.engine import TencryptAuthResult
        self.calls.append((name, len(msgs[0])))
        self._one_length(msgs)
        assert all(len(s) == 32 for s in seeds) and len(seeds) == len(msgs) == len(rounds)
        cts = [A.encrypt(self._base(r), s, m) for r, s, m in zip(rounds, seeds, msgs)]
        for (u, _, _), s, m in zip(cts, seeds, msgs):
            self.scalars[u] = A.h3(s, m)
        return TencryptAuthResult([True] * len(cts), [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts])

    def _open_one(self, sig, u, v, w):
        sig = bytes(sig)
        if sig not in self.bases:
            self.bases[sig] = T.gt_base(O.g2_decompress(sig))
        c = T.g1_class(u)
        if c:
            return c, None
        m = A.open_tail(T.encode_gt(T.gt_pow(self.bases[sig], self.scalars[bytes(u)])), u, v, w)
        return (0, m) if m is not None else (A.REJ_TLOCK_AUTH, None)

    def tlock_decrypt_auth(self, sig, us, vs, ws, kdf=1):
        from drand_amd.engine import TdecryptAuthResult
        self.calls.append(("tlock_decrypt_auth", len(ws[0])))
        self._one_length(ws)
        got = [self._open_one(sig, u, v, w) for u, v, w in zip(us, vs, ws)]
        return TdecryptAuthResult([c == 0 for c, _ in got], [c for c, _ in got], [m for _, m in got])

    def tlock_decrypt_auth_rounds(self, sigs, us_per_round, vs_per_round, ws_per_round, kdf=1):
        from drand_amd.engine import TdecryptAuthRoundsResult
        flat = [w for run in ws_per_round for w in run]
        self.calls.append(("tlock_decrypt_auth_rounds", len(flat[0])))
        self._one_length(flat)
        got = [self._open_one(s, u, v, w) for s, us, vs, ws in zip(sigs, us_per_round, vs_per_round, ws_per_round)
               for u, v, w in zip(us, vs, ws)]
        return TdecryptAuthRoundsResult([c == 0 for c, _ in got], [c for c, _ in got], [m for _, m in got], [0] * len(sigs))


RAGGED = [b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100)), bytes(range(33)), b"\xa5", bytes(32)]
SEEDS = [A.seed_of(500 + i) for i in range(len(RAGGED))]


@pytest.fixture(scope="module")
def sig():
    return C.sign(SK, O.message_v2(ROUND))


@pytest.fixture()
def stand_in():
    return AuthStandIn(O.g1_compress(O.sk_to_pk(SK)), {})


def test_callers_group_by_length_and_keep_the_input_order(stand_in, sig):
    cts = callers.timelock_encrypt_auth(stand_in, ROUND, RAGGED, seeds=SEEDS)
    assert stand_in.calls == [("tlock_encrypt_auth", n) for n in (1, 32, 100, 33)]  # one call per distinct length
    base = stand_in._base(ROUND)
    assert cts == [A.encrypt(base, s, m) for s, m in zip(SEEDS, RAGGED)]
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, cts) == RAGGED
    assert stand_in.calls == [("tlock_decrypt_auth", n) for n in (1, 32, 100, 33)], "verify=False: no verify_unchained call"
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, cts, verify=True) == RAGGED
    assert stand_in.calls[0] == "verify_unchained" and stand_in.calls.count("verify_unchained") == 1
    # fresh seeds when none are given: 32 bytes each, all distinct, and the ciphertexts still open
    fresh = callers.timelock_encrypt_auth(stand_in, ROUND, RAGGED[:2])
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, fresh) == RAGGED[:2] and fresh != cts[:2]


def test_callers_rounds_forms(stand_in, sig):
    items = [(ROUND, m) for m in RAGGED]
    cts = callers.timelock_encrypt_auth_rounds(stand_in, items, seeds=SEEDS)
    assert cts == callers.timelock_encrypt_auth(stand_in, ROUND, RAGGED, seeds=SEEDS)
    stand_in.calls.clear()
    runs = [(ROUND, sig, cts[:1]), (ROUND, sig, cts[1:4]), (ROUND, sig, cts[4:])]
    assert callers.timelock_decrypt_auth_rounds(stand_in, runs) == [RAGGED[:1], RAGGED[1:4], RAGGED[4:]]
    assert "verify_unchained" not in stand_in.calls and len(stand_in.calls) == 4
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth_rounds(stand_in, runs, verify=True) == [RAGGED[:1], RAGGED[1:4], RAGGED[4:]]
    assert stand_in.calls[0] == "verify_unchained" and stand_in.calls.count("verify_unchained") == 1
    with pytest.raises(callers.VerifyError):
        callers.timelock_decrypt_auth_rounds(stand_in, [(ROUND + 1, sig, cts[:1])], verify=True)


def test_callers_refuse_empty_and_long_messages(stand_in, sig):
    for bad in (b"", bytes(257)):
        with pytest.raises(ValueError):
            callers.timelock_encrypt_auth(stand_in, ROUND, [b"ok", bad])
        with pytest.raises(ValueError):
            callers.timelock_encrypt_auth_rounds(stand_in, [(ROUND, b"ok"), (ROUND, bad)])
        with pytest.raises(ValueError):
            callers.timelock_decrypt_auth(stand_in, ROUND, sig, [(T.u_of(2), bytes(32), bad)])
        with pytest.raises(ValueError):
            callers.timelock_decrypt_auth_rounds(stand_in, [(ROUND, sig, [(T.u_of(2), bytes(32), bad)])])
    assert stand_in.calls == []
    with pytest.raises(ValueError):
        callers.timelock_encrypt_auth(stand_in, ROUND, RAGGED, seeds=SEEDS[:3])


def test_callers_give_none_for_failed_items(stand_in, sig):
    cts = callers.timelock_encrypt_auth(stand_in, ROUND, RAGGED, seeds=SEEDS)
    bad = list(cts)
    bad[1] = (cts[1][0], flip(cts[1][1], 3), cts[1][2])  # a V bit
    bad[2] = (cts[2][0], cts[2][1], flip(cts[2][2], 99))  # the last W byte
    bad[3] = (cts[3][0][:47], cts[3][1], cts[3][2])  # a 47-byte U: rejected host-side
    bad[4] = (T.bad_us()[O.REJ_NOT_ON_CURVE], cts[4][1], cts[4][2])
    want = [RAGGED[0], None, None, None, None, RAGGED[5]]
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, bad) == want
    assert callers.timelock_decrypt_auth_rounds(stand_in, [(ROUND, sig, bad[:2]), (ROUND, sig, bad[2:])]) == [want[:2], want[2:]]
    # the wrong round's signature: every item None, and no exception
    other = C.sign(SK, O.message_v2(ROUND + 1))
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, other, cts) == [None] * len(cts)
    assert "verify_unchained" not in stand_in.calls
    with pytest.raises(callers.VerifyError):
        callers.timelock_decrypt_auth(stand_in, ROUND, other, cts, verify=True)
