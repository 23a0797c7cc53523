"""The fused tail of timelock encrypt / decrypt on the host build (tools/opcount tmask: drand_amd/csrc/tmask.h
compiled with -DBLS_HOST, the midstate, the counter blocks and the stores as k_tmask.hip runs them) against
callers.kdf_sha256_ctr, and the callers.timelock_decrypt / timelock_encrypt family on a stand-in engine backed
by the oracle. No GPU.

Expected bytes are m XOR kdf_sha256_ctr(encode_gt(K), mlen) with K from one oracle pairing for the module.
"""
import json
import os
import subprocess

import pytest

from drand_amd import callers
from oracle import bls12381 as O
from oracle import c_oracle as C
from tests.support import tlock_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9011223344556677889900AABBCCDD
ROUND = 7
R1 = 0x5B1E7C0FFEE0DDBA11AD5EED0123456789ABCDEF0FEDCBA9876543210F1E2D3C % O.R
R2 = (O.R - 0x1234567) % O.R  # full width, top bits set
# both sides of a key-stream block (32) and of a SHA block (64), and the cap
MLENS = [1, 3, 31, 32, 33, 63, 64, 65, 255, 256]


@pytest.fixture(scope="module")
def opcount_bin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "opcount"], check=True, capture_output=True)
    return os.path.join(ROOT, "tools", "opcount")


@pytest.fixture(scope="module")
def sig():
    return C.sign(SK, O.message_v2(ROUND))


@pytest.fixture(scope="module")
def base(sig):
    # ONE oracle pairing for the module: e(G1, sigma)^3 = e(pk, H(MessageV2(ROUND)))^3, the sealing base too
    return T.gt_base(O.g2_decompress(sig, check_subgroup=False))


@pytest.fixture(scope="module")
def gts(base):
    return [T.GT_ONE, T.encode_gt(base), T.encode_gt(T.gt_pow(base, R2))]


def message(k, mlen):
    return bytes((37 * k + 11 * j + 5) % 256 for j in range(mlen))


def xor(a, b):
    assert len(a) == len(b)
    return bytes(x ^ y for x, y in zip(a, b))


def run_tmask(binp, mlen, items):
    """items: (gt576, msg, class)"""
    text = "%d\n" % mlen + "".join("%s %s %d\n" % (g.hex(), m.hex(), c) for g, m, c in items)
    r = subprocess.run([binp, "tmask"], input=text, capture_output=True, text=True)
    assert r.stdout, r.stderr
    return r.returncode, json.loads(r.stdout)


@pytest.mark.parametrize("mlen", MLENS)
def test_masked_bytes_match_the_python_kdf(opcount_bin, gts, mlen):
    msgs = [message(k, mlen) for k in range(3)]
    rc, out = run_tmask(opcount_bin, mlen, [(g, m, 0) for g, m in zip(gts, msgs)])
    assert rc == 0 and out["mlen"] == mlen and out["forms_match"] is True
    want = [xor(m, callers.kdf_sha256_ctr(g, mlen)) for g, m in zip(gts, msgs)]
    assert [bytes.fromhex(x) for x in out["out"]] == want


@pytest.mark.parametrize("mlen", [3, 32])
def test_a_rejected_item_gets_zeros_and_its_neighbours_their_bytes(opcount_bin, gts, mlen):
    msgs = [message(k, mlen) for k in range(3)]
    rc, out = run_tmask(opcount_bin, mlen, [(gts[0], msgs[0], 0), (gts[1], msgs[1], 5), (gts[2], msgs[2], 0)])
    assert rc == 0 and out["forms_match"] is True
    want = [xor(msgs[0], callers.kdf_sha256_ctr(gts[0], mlen)), bytes(mlen),
            xor(msgs[2], callers.kdf_sha256_ctr(gts[2], mlen))]
    assert [bytes.fromhex(x) for x in out["out"]] == want


def test_tool_refuses_lengths_outside_the_cap(opcount_bin, gts):
    for mlen in (0, 257):
        r = subprocess.run([opcount_bin, "tmask"], input="%d\n" % mlen, capture_output=True, text=True)
        assert r.returncode == 2 and not r.stdout


# ------------------------------------------------------------------ the callers, stand-in engine
class FusedStandIn(T.OracleTlockEngine):
    """The oracle stand-in with the fused Engine methods beside the raw ones: every value is base^r for a
    known r (one round, ROUND, under the module's key)."""

    def __init__(self, pk48, scalars, base):
        super().__init__(pk48, scalars)
        self.base = base

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
        return lens.pop()

    def _open(self, sig, us):
        res = super().tlock_open(sig, us)
        self.calls.pop()
        return res

    def tlock_decrypt(self, sig, us, cs, kdf=1):
        from drand_amd.engine import TdecryptResult
        self.calls.append("tlock_decrypt")
        mlen = self._one_length(cs)
        res = self._open(sig, us)
        return TdecryptResult(res.ok, res.reject_class,
                              [None if g is None else xor(c, callers.kdf_sha256_ctr(g, mlen)) for g, c in zip(res.gt, cs)])

    def tlock_decrypt_rounds(self, sigs, us_per_round, cs_per_round, kdf=1):
        from drand_amd.engine import TdecryptRoundsResult
        self.calls.append("tlock_decrypt_rounds")
        mlen = self._one_length([c for run in cs_per_round for c in run])
        ok, cls, msgs = [], [], []
        for s, us, cs in zip(sigs, us_per_round, cs_per_round):
            res = self._open(s, us)
            ok += res.ok
            cls += res.reject_class
            msgs += [None if g is None else xor(c, callers.kdf_sha256_ctr(g, mlen)) for g, c in zip(res.gt, cs)]
        return TdecryptRoundsResult(ok, cls, msgs, [0] * len(sigs))

    def tlock_open_rounds(self, sigs, us_per_round):
        from drand_amd.engine import TlockRoundsResult
        self.calls.append("tlock_open_rounds")
        parts = [self._open(s, us) for s, us in zip(sigs, us_per_round)]
        return TlockRoundsResult([x for p in parts for x in p.ok], [x for p in parts for x in p.reject_class],
                                 [x for p in parts for x in p.gt], [0] * len(sigs))

    def tlock_seal(self, round_, scalars, pk48=None):
        from drand_amd.engine import TsealResult
        self.calls.append("tlock_seal")
        assert round_ == ROUND
        return TsealResult([True] * len(scalars), [T.u_of(k) for k in scalars],
                           [T.encode_gt(T.gt_pow(self.base, k)) for k in scalars])

    def tlock_seal_rounds(self, rounds, scalars, pk48=None):
        res = self.tlock_seal(ROUND, scalars, pk48)
        self.calls[-1] = "tlock_seal_rounds"
        assert set(rounds) <= {ROUND}
        return res

    def tlock_encrypt(self, round_, scalars, msgs, pk48=None, kdf=1):
        from drand_amd.engine import TencryptResult
        self.calls.append("tlock_encrypt")
        assert round_ == ROUND
        mlen = self._one_length(msgs)
        return TencryptResult([True] * len(scalars), [T.u_of(k) for k in scalars],
                              [xor(m, callers.kdf_sha256_ctr(T.encode_gt(T.gt_pow(self.base, k)), mlen))
                               for k, m in zip(scalars, msgs)])

    def tlock_encrypt_rounds(self, rounds, scalars, msgs, pk48=None, kdf=1):
        assert set(rounds) <= {ROUND}
        res = self.tlock_encrypt(ROUND, scalars, msgs, pk48)
        self.calls[-1] = "tlock_encrypt_rounds"
        return res


RS = [3, 5, R1, 11]
RAGGED = [b"\x5a", bytes(range(32)), bytes((7 * i + 3) % 256 for i in range(100)), bytes(range(33))]


@pytest.fixture()
def stand_in(base):
    pk = O.g1_compress(O.sk_to_pk(SK))
    return FusedStandIn(pk, {T.u_of(r): r for r in RS}, base)


def expected_cts(base, msgs, rs):
    return [(T.u_of(r), xor(m, callers.kdf_sha256_ctr(T.encode_gt(T.gt_pow(base, r)), len(m)))) for m, r in zip(msgs, rs)]


def test_ragged_lengths_are_padded_and_cut_back(stand_in, sig, base):
    cts = expected_cts(base, RAGGED, RS)
    assert callers.timelock_encrypt(stand_in, ROUND, RAGGED, scalars=RS) == cts
    assert stand_in.calls == ["tlock_encrypt"]
    stand_in.calls.clear()
    assert callers.timelock_decrypt(stand_in, ROUND, sig, cts) == RAGGED
    assert stand_in.calls == ["verify_unchained", "tlock_decrypt"]
    # the same bytes as the unfused callers give
    stand_in.calls.clear()
    assert callers.timelock_seal(stand_in, ROUND, RAGGED, callers.kdf_sha256_ctr, scalars=RS) == cts
    assert callers.timelock_open(stand_in, ROUND, sig, cts, callers.kdf_sha256_ctr, verify=False) == RAGGED


def test_a_300_byte_message_and_an_empty_one_take_the_existing_functions(stand_in, sig, base):
    for extra in (bytes((3 * i) % 256 for i in range(300)), b""):
        msgs = RAGGED[:3] + [extra]
        cts = expected_cts(base, msgs, RS)
        stand_in.calls.clear()
        assert callers.timelock_encrypt(stand_in, ROUND, msgs, scalars=RS) == cts
        assert callers.timelock_decrypt(stand_in, ROUND, sig, cts, verify=False) == msgs
        assert callers.timelock_encrypt_rounds(stand_in, [(ROUND, m) for m in msgs], scalars=RS) == cts
        assert callers.timelock_decrypt_rounds(stand_in, [(ROUND, sig, cts)], verify=False) == [msgs]
        assert stand_in.calls == ["tlock_seal", "tlock_open", "tlock_seal_rounds", "tlock_open_rounds"]


def test_a_47_byte_u_is_none_and_the_beacon_is_checked_first(stand_in, sig, base):
    cts = expected_cts(base, RAGGED, RS)
    cts.insert(1, (T.u_of(3)[:47], b"short U"))
    cts.append((T.bad_us()[O.REJ_NOT_ON_CURVE], b"whatever"))
    want = [RAGGED[0], None] + RAGGED[1:] + [None]
    assert callers.timelock_decrypt(stand_in, ROUND, sig, cts) == want
    assert callers.timelock_decrypt_rounds(stand_in, [(ROUND, sig, cts[:2]), (ROUND, sig, cts[2:])]) == [want[:2], want[2:]]
    stand_in.calls.clear()
    with pytest.raises(callers.VerifyError) as ei:
        callers.timelock_decrypt(stand_in, ROUND + 1, sig, cts)
    assert ei.value.round == ROUND + 1 and stand_in.calls == ["verify_unchained"]
    with pytest.raises(callers.VerifyError):
        callers.timelock_decrypt_rounds(stand_in, [(ROUND, sig, cts[:2]), (ROUND + 1, sig, cts[2:])])


def test_encrypt_then_decrypt_round_trips(stand_in, sig, base):
    cts = callers.timelock_encrypt(stand_in, ROUND, RAGGED, scalars=RS)
    assert callers.timelock_decrypt(stand_in, ROUND, sig, cts) == RAGGED
    items = [(ROUND, m) for m in RAGGED]
    cts_r = callers.timelock_encrypt_rounds(stand_in, items, scalars=RS)
    assert cts_r == cts
    assert callers.timelock_decrypt_rounds(stand_in, [(ROUND, sig, cts_r[:1]), (ROUND, sig, cts_r[1:])]) == [RAGGED[:1],
                                                                                                               RAGGED[1:]]
    with pytest.raises(ValueError):
        callers.timelock_encrypt(stand_in, ROUND, RAGGED, scalars=RS[:3])
