"""The authenticated timelock's ragged forms (blsv_tlock_*_auth*_var: a length per item, the bytes packed back to
back) on the host. No GPU.

- tools/opcount tauthv: tauth.h's forms over a packed batch whose spans come from a table of prefix offsets
  (tauth_span_ragged, as k_tauth.hip's ragged kernels take them), against tests/support/tauth_ref.py (hashlib and
  Python integers): the full length list, the dword and the byte form, in place.
- tools/tauthvar-asan: the guard, the offsets, the pass slices and the three layouts of hostlogic.h, a stand-alone
  program under ASan + UBSan, against values computed by hand here.
- callers.timelock_*_auth*(ragged=True) on a stand-in engine that has the _var methods, answered by tauth_ref.

The tool's tails take K / E as given bytes, so its cases need no pairing.
"""
import json
import os
import random
import subprocess

import pytest

from drand_amd import callers
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import tauth_ref as A
from tests.support import tlock_ref as T
from tests.test_tauth_host import ROUND, SK, AuthStandIn, flip, some_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tauth_ref.MLENS and the edges of the ragged form (the hashed length is 52 + mlen): 48 + mlen fills a block;
# piece and H4 block edges; the padding spills into a second block. Shuffled so that neighbours differ.
EDGES = [15, 16, 17, 79, 80, 81, 31, 32, 33, 63, 64, 65, 131, 132, 195, 196]
LENS = sorted(set(A.MLENS) | set(EDGES))
random.Random(20240607).shuffle(LENS)
DWORD_LENS = list(A.DWORD_LENS) + [16, 80, 64, 132, 196]
random.Random(7).shuffle(DWORD_LENS)


def build(target):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "tools", target)


@pytest.fixture(scope="module")
def opcount_bin():
    return build("opcount")


@pytest.fixture(scope="module")
def tauthvar_bin():
    return build("tauthvar-asan")


def run_tauthv(binp, lines):
    r = subprocess.run([binp, "tauthv"], input="0\n" + "".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


# ------------------------------------------------------------------ opcount tauthv
def cases_of(lens):
    return [(A.seed_of(7000 + i), A.message(i, n), some_gt(i % 7)) for i, n in enumerate(lens)]


def check_ragged(binp, lens, dword_forms):
    cases = cases_of(lens)
    want, lines = [], []
    for seed, msg, gt in cases:
        k = A.h3(seed, msg)
        v, w = A.seal_tail(seed, msg, gt)
        want.append((k, v, w))
        lines.append("seal %s %s %s" % (seed.hex(), msg.hex(), gt.hex()))
        lines.append("open %s %s %s %s" % (gt.hex(), A.u_of(k).hex(), v.hex(), w.hex()))
    rc, out = run_tauthv(binp, lines)
    # the byte form, the dword form where every length allows it, and both in place agree; every guard is intact
    assert rc == 0 and out["forms_match"] is True and out["dword_forms"] == dword_forms
    assert len(out["seal"]) == len(out["open"]) == len(cases)
    for (k, v, w), got in zip(want, out["seal"]):
        assert got["ok"] == 1 and int(got["k"], 16) == k
        assert bytes.fromhex(got["v"]) == v and bytes.fromhex(got["w"]) == w
    for (seed, msg, gt), got in zip(cases, out["open"]):
        assert got["cls"] == 0 and bytes.fromhex(got["msg"]) == msg


def test_tauthv_full_length_list_byte_form(opcount_bin):
    assert len(LENS) >= 25 and any(n % 4 for n in LENS)
    check_ragged(opcount_bin, LENS + LENS[::-1][:5], 0)


def test_tauthv_dword_lengths_run_the_dword_form_too(opcount_bin):
    assert all(n % 4 == 0 for n in DWORD_LENS)
    check_ragged(opcount_bin, DWORD_LENS, 2)


def test_tauthv_failing_items_get_their_own_length_of_zeros(opcount_bin):
    lens = [33, 1, 64, 17, 256, 4, 80]
    cts = []
    for seed, msg, gt in cases_of(lens):
        k = A.h3(seed, msg)
        v, w = A.seal_tail(seed, msg, gt)
        cts.append([gt, A.u_of(k), v, w, 0, msg])
    cts[1][3] = flip(cts[1][3], 0)  # the one W byte of a 1-byte item
    cts[2][2] = flip(cts[2][2], 9, 0x04)  # a V bit
    cts[4][3] = flip(cts[4][3], 255, 0x80)  # the last W byte of the longest item
    cts[5][4] = 5  # arrives with a decode class
    bad = {1: A.REJ_TLOCK_AUTH, 2: A.REJ_TLOCK_AUTH, 4: A.REJ_TLOCK_AUTH, 5: 5}
    rc, out = run_tauthv(opcount_bin, ["open %s %s %s %s %d" % (g.hex(), u.hex(), v.hex(), w.hex(), c)
                                       for g, u, v, w, c, _ in cts])
    assert rc == 0 and out["forms_match"] is True
    for i, (ct, got) in enumerate(zip(cts, out["open"])):
        assert got["cls"] == bad.get(i, 0), i
        assert bytes.fromhex(got["msg"]) == (bytes(lens[i]) if i in bad else ct[5]), i  # neighbours untouched
        if i != 5:
            assert A.open_tail(*ct[:4]) == (None if i in bad else ct[5]), i


def test_tauthv_refuses_a_length_outside_the_cap_and_the_old_header(opcount_bin):
    seed, gt = A.seed_of(1), some_gt(0)
    for msg in (b"", bytes(257)):
        r = subprocess.run([opcount_bin, "tauthv"], input="0\nseal %s %s %s\n" % (seed.hex(), msg.hex(), gt.hex()),
                           capture_output=True, text=True)
        assert r.returncode == 2 and not r.stdout
    r = subprocess.run([opcount_bin, "tauthv"], input="32\n", capture_output=True, text=True)
    assert r.returncode == 2 and not r.stdout


# ------------------------------------------------------------------ the guard, the offsets, the layouts (ASan + UBSan)
def run_var(binp, cap, lens):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([binp, str(cap)] + [str(n) for n in lens], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def up8(v):
    return (v + 7) & ~7


def up64(v):
    return (v + 63) & ~63


def layout_by_hand(cnt, nbytes):
    o_in = 64 * cnt
    secret = up8(o_in + nbytes)
    o_out = secret + (8 + 48 + 32) * cnt
    o_flag = up8(o_out + nbytes)
    o_offs = up8(o_flag + cnt)
    return [o_in, secret, o_out, o_flag, o_offs, o_offs + 4 * (cnt + 1)]


def test_offsets_totals_and_pass_slices_by_hand(tauthvar_bin):
    out = run_var(tauthvar_bin, 2, [1, 32, 100, 33, 32])
    assert out["fits"] is True and out["total"] == 198
    assert out["passes"] == [
        [0, 2, 0, 33, False, [0, 1, 33], [128, 168, 344, 384, 392, 404]],
        [2, 2, 33, 133, False, [0, 100, 133], [128, 264, 440, 576, 584, 596]],
        [4, 1, 166, 32, True, [0, 32], [64, 96, 184, 216, 224, 232]],
    ]
    for base, cnt, at, nbytes, words, offs, layout in out["passes"]:
        assert layout == layout_by_hand(cnt, nbytes)
    # the latency layouts of the 5 items, 198 bytes: one signature, then 7 with two of them idle
    n, total = 5, 198
    o_offs = 96 + 80 * n
    assert out["lat_open"][0] == [o_offs, o_offs + 24, o_offs + 24 + total, up64(o_offs + 24 + total),
                                  up64(o_offs + 24 + total) + total, up64(o_offs + 24 + total) + total + n,
                                  up64(o_offs + 24 + total) + total + n + 1]
    o_offs = 96 * 7 + 84 * n + 8
    assert out["lat_open"][1][:3] == [o_offs, o_offs + 24, o_offs + 24 + total]
    assert out["lat_open"][1][6] == up64(o_offs + 24 + total) + total + n + 7
    assert out["lat_seal"][0] == [0, 24, 24 + 160, 184 + total, up64(184 + total), up64(184 + total) + 80 * n,
                                  up64(184 + total) + 80 * n + total, up64(184 + total) + 80 * n + total + n]
    assert out["lat_seal"][1][:4] == [40, 64, 224, 224 + total]


def test_one_pass_dword_lengths_and_the_longest_items(tauthvar_bin):
    out = run_var(tauthvar_bin, 16384, [4, 8, 256, 12])
    assert out["total"] == 280 and out["passes"] == [[0, 4, 0, 280, True, [0, 4, 12, 268, 280], layout_by_hand(4, 280)]]
    lens = [256] * 65 + [1]
    out = run_var(tauthvar_bin, 64, lens)
    assert out["total"] == 65 * 256 + 1
    assert [p[:5] for p in out["passes"]] == [[0, 64, 0, 64 * 256, True], [64, 2, 64 * 256, 257, False]]
    assert out["passes"][1][5] == [0, 256, 257]
    out = run_var(tauthvar_bin, 3, [])
    assert out["fits"] is True and out["total"] == 0 and out["passes"] == [] and "lat_open" not in out


@pytest.mark.parametrize("lens", [[0], [257], [5, 0, 5], [5, 6, 257, 7], [1, 2, 3, 2 ** 32 - 1]])
def test_one_bad_length_anywhere_is_refused(tauthvar_bin, lens):
    out = run_var(tauthvar_bin, 2, lens)
    assert out["fits"] is False and "passes" not in out  # and the program checked that *total was not written


def test_overflow_guards_at_size_max_scale_counts(tauthvar_bin):
    out = run_var(tauthvar_bin, 2, [1])
    # n = SIZE_MAX / 1024 + 1, SIZE_MAX and SIZE_MAX / 256 are refused before a length is read; a null table with
    # n = 1; n = 0 reads nothing and fits; tauth_fits' own edge. Then the latency layouts' eight refusals.
    assert out["refused"] == [True] * 6 and out["lat_refused"] == [True] * 8


# ------------------------------------------------------------------ the callers, stand-in engine
class VarStandIn(AuthStandIn):
    """AuthStandIn with the four _var methods: any lengths in one call, answered item by item by tauth_ref."""

    @staticmethod
    def _lengths_ok(items):
        assert all(1 <= len(x) <= 256 for x in items)

    def tlock_encrypt_auth_var(self, round_, seeds, msgs, pk48=None, kdf=1):
        return self.tlock_encrypt_auth_rounds_var([round_] * len(msgs), seeds, msgs, pk48, kdf, name="tlock_encrypt_auth_var")

    def tlock_encrypt_auth_rounds_var(self, rounds, seeds, msgs, pk48=None, kdf=1, name="tlock_encrypt_auth_rounds_var"):
        from drand_amd.engine import TencryptAuthResult
        self.calls.append((name, [len(m) for m in msgs]))
        self._lengths_ok(msgs)
        cts = [A.encrypt(self._base(r), s, m) for r, s, m in zip(rounds, seeds, msgs)]
        for (u, _, _), s, m in zip(cts, seeds, msgs):
            self.scalars[u] = A.h3(s, m)
        return TencryptAuthResult([True] * len(cts), [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts])

    def tlock_decrypt_auth_var(self, sig, us, vs, ws, kdf=1):
        from drand_amd.engine import TdecryptAuthResult
        self.calls.append(("tlock_decrypt_auth_var", [len(w) for w in ws]))
        self._lengths_ok(ws)
        got = [self._open_one(sig, u, v, w) for u, v, w in zip(us, vs, ws)]
        return TdecryptAuthResult([c == 0 for c, _ in got], [c for c, _ in got], [m for _, m in got])

    def tlock_decrypt_auth_rounds_var(self, sigs, us_per_round, vs_per_round, ws_per_round, kdf=1):
        from drand_amd.engine import TdecryptAuthRoundsResult
        self.calls.append(("tlock_decrypt_auth_rounds_var", [[len(w) for w in run] for run in ws_per_round]))
        self._lengths_ok([w for run in ws_per_round for w in run])
        got = [self._open_one(s, u, v, w) for s, us, vs, ws in zip(sigs, us_per_round, vs_per_round, ws_per_round)
               for u, v, w in zip(us, vs, ws)]
        return TdecryptAuthRoundsResult([c == 0 for c, _ in got], [c for c, _ in got], [m for _, m in got], [0] * len(sigs))


MSGS = [b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100)), bytes(range(33)), bytes(32)]
LENGTHS = [1, 32, 100, 33, 32]
SEEDS = [A.seed_of(900 + i) for i in range(len(MSGS))]


@pytest.fixture(scope="module")
def sig():
    return C.sign(SK, O.message_v2(ROUND))


@pytest.fixture()
def stand_in():
    return VarStandIn(O.g1_compress(O.sk_to_pk(SK)), {})


def test_ragged_callers_make_one_engine_call_and_keep_the_order(stand_in, sig):
    assert [len(m) for m in MSGS] == LENGTHS
    cts = callers.timelock_encrypt_auth(stand_in, ROUND, MSGS, seeds=SEEDS, ragged=True)
    assert stand_in.calls == [("tlock_encrypt_auth_var", LENGTHS)]  # ONE call, every length in it, in input order
    base = stand_in._base(ROUND)
    assert cts == [A.encrypt(base, s, m) for s, m in zip(SEEDS, MSGS)]
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, cts, ragged=True) == MSGS
    assert stand_in.calls == [("tlock_decrypt_auth_var", LENGTHS)]
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, cts, verify=True, ragged=True) == MSGS
    assert stand_in.calls == ["verify_unchained", ("tlock_decrypt_auth_var", LENGTHS)]


def test_ragged_callers_rounds_forms(stand_in, sig):
    cts = callers.timelock_encrypt_auth_rounds(stand_in, [(ROUND, m) for m in MSGS], seeds=SEEDS, ragged=True)
    assert stand_in.calls == [("tlock_encrypt_auth_rounds_var", LENGTHS)]
    assert cts == [A.encrypt(stand_in._base(ROUND), s, m) for s, m in zip(SEEDS, MSGS)]
    stand_in.calls.clear()
    runs = [(ROUND, sig, cts[:1]), (ROUND, sig, []), (ROUND, sig, cts[1:4]), (ROUND, sig, cts[4:])]
    assert callers.timelock_decrypt_auth_rounds(stand_in, runs, ragged=True) == [MSGS[:1], [], MSGS[1:4], MSGS[4:]]
    assert stand_in.calls == [("tlock_decrypt_auth_rounds_var", [[1], [], [32, 100, 33], [32]])]


def test_ragged_callers_give_none_for_host_side_rejects_and_failed_items(stand_in, sig):
    cts = callers.timelock_encrypt_auth(stand_in, ROUND, MSGS, seeds=SEEDS, ragged=True)
    bad = list(cts)
    bad[1] = (cts[1][0], flip(cts[1][1], 3), cts[1][2])  # a V bit: the engine's verdict
    bad[2] = (cts[2][0][:47], cts[2][1], cts[2][2])  # a 47-byte U: rejected host-side, never sent
    bad[3] = (cts[3][0], cts[3][1] + b"\x00", cts[3][2])  # a 33-byte V: rejected host-side
    want = [MSGS[0], None, None, None, MSGS[4]]
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, bad, ragged=True) == want
    assert stand_in.calls == [("tlock_decrypt_auth_var", [1, 32, 32])]
    stand_in.calls.clear()
    got = callers.timelock_decrypt_auth_rounds(stand_in, [(ROUND, sig, bad[:2]), (ROUND, sig, bad[2:])], ragged=True)
    assert got == [want[:2], want[2:]]
    assert stand_in.calls == [("tlock_decrypt_auth_rounds_var", [[1, 32], [32]])]
    # nothing to send: no engine call at all
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, [bad[2]], ragged=True) == [None]
    assert callers.timelock_encrypt_auth(stand_in, ROUND, [], seeds=[], ragged=True) == []
    assert stand_in.calls == []
    for wrong in (b"", bytes(257)):
        with pytest.raises(ValueError):
            callers.timelock_encrypt_auth(stand_in, ROUND, [b"ok", wrong], ragged=True)
    assert stand_in.calls == []


def test_the_default_still_groups_by_length(stand_in, sig):
    cts = callers.timelock_encrypt_auth(stand_in, ROUND, MSGS, seeds=SEEDS)
    assert stand_in.calls == [("tlock_encrypt_auth", n) for n in (1, 32, 100, 33)]
    assert cts == callers.timelock_encrypt_auth(stand_in, ROUND, MSGS, seeds=SEEDS, ragged=True)  # the same ciphertexts
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth(stand_in, ROUND, sig, cts, ragged=False) == MSGS
    assert stand_in.calls == [("tlock_decrypt_auth", n) for n in (1, 32, 100, 33)]
    stand_in.calls.clear()
    assert callers.timelock_decrypt_auth_rounds(stand_in, [(ROUND, sig, cts)]) == [MSGS]
    assert stand_in.calls == [("tlock_decrypt_auth_rounds", n) for n in (1, 32, 100, 33)]
    stand_in.calls.clear()
    callers.timelock_encrypt_auth_rounds(stand_in, [(ROUND, m) for m in MSGS], seeds=SEEDS)
    assert stand_in.calls == [("tlock_encrypt_auth_rounds", n) for n in (1, 32, 100, 33)]
