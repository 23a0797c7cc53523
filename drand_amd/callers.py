"""Batched rewrites of drand's two serial verification loops.

The reference walks a chain one round at a time, with one full BLS verify per round:

* ``verifyingClient.getTrustedPreviousSignature`` (client/verify.go:115-174) fetches rounds
  ``trust+1 .. round-1`` and calls ``chain.VerifyBeacon`` on each (verify.go:146-163).
* ``verifyingClient.verify`` (client/verify.go:176-208) then checks the requested round, V1 or V2
  depending on ``v2from``, and sets ``Random = sha256(sig)`` (chain/beacon.go:66-75).
* ``syncer.tryNode`` (chain/beacon/sync.go:83-131) streams ``BeaconPacket``s, verifies each
  (sync.go:105) and appends it through ``appendStore.Put`` (chain/beacon/store.go:40-54), which
  checks ``Round == last.Round+1`` and ``PreviousSig == last.Signature``.

Here both loops keep their observable behaviour (same accepted prefix, same first failing round,
same point-of-trust update, same error kinds) but hand whole ranges to the GPU engine in one
``Engine.verify_chained`` call per chunk. Fetching and storing stay with the caller (network and
storage are out of scope); the callables passed in stand for ``indirectClient.Get`` and
``chain.Store.Put``.

Every verdict comes from the HIP kernels through the C ABI; there is no CPU verify here.
"""
from __future__ import annotations

import hashlib
import threading
from dataclasses import dataclass
from typing import Callable, Iterable, Optional

UINT64_MAX = 2 ** 64 - 1
SIG_LEN = 96


class VerifyError(Exception):
    """A beacon failed verification (kyber's "bls: invalid signature" or a decode error)."""

    def __init__(self, round_, msg):
        super().__init__(msg)
        self.round = round_


class FetchError(Exception):
    """``indirectClient.Get`` failed for a round (client/verify.go:149-152)."""

    def __init__(self, round_, cause):
        super().__init__(f"could not get round {round_}: {cause}")
        self.round = round_
        self.__cause__ = cause


@dataclass
class ChainInfo:
    """The two fields of ``chain.Info`` the walk uses (chain/info.go): G1 public key (48 B
    compressed) and ``GroupHash``, which is the previous signature of round 1
    (client/verify.go:122-124)."""
    public_key: bytes
    group_hash: bytes


@dataclass
class RandomData:
    """``client.RandomData`` (client/random.go:5-12). ``version`` is 2 once ``round >= v2from``."""
    round: int
    signature: bytes = b""
    previous_signature: Optional[bytes] = None
    signature_v2: bytes = b""
    randomness: bytes = b""
    version: int = 1

    def sig(self):
        return self.signature_v2 if self.version == 2 else self.signature


@dataclass
class Beacon:
    """``chain.Beacon`` (chain/beacon.go:16-25)."""
    previous_sig: bytes
    round: int
    signature: bytes
    signature_v2: bytes = b""


def randomness_from_signature(sig: bytes) -> bytes:
    """``chain.RandomnessFromSignature`` (chain/beacon.go:66-69): sha256 of the signature bytes.
    Host-side, like the reference: it runs only after the GPU verdict accepted the beacon."""
    return hashlib.sha256(sig).digest()


def _verify_run(engine, first_round, prev0, sigs, fast=False):
    """Verify ``sigs`` as consecutive rounds starting at ``first_round`` whose first previous
    signature is ``prev0``. Returns the index of the first rejected beacon, or None.

    ``fast=True`` hands the range to ``Engine.verify_chained_rlc`` (opt-in randomized batch
    verification: same rejects, acceptance of a bad round with probability at most 2^-64,
    include/blsverify.h); the default is the exact check.

    A wrong-length signature is a reject in the reference (kyber's unmarshal fails); the engine
    refuses such input host-side, so the run is cut there and that index is reported."""
    n = len(sigs)
    cut = next((i for i, s in enumerate(sigs) if len(s) != SIG_LEN), n)
    if cut and len(prev0) not in (32, 96):
        # Only the first round's prev may be another length; the C ABI takes 32 or 96 bytes.
        # A kyber verify of such a message is still well defined, so route it through the
        # message-form entry point.
        first = engine.verify_messages([hashlib.sha256(bytes(prev0) + first_round.to_bytes(8, "big")).digest()],
                                       [sigs[0]])
        if not first.ok[0]:
            return 0
        rest = _verify_run(engine, first_round + 1, sigs[0], sigs[1:cut], fast)
        return None if rest is None else rest + 1
    if cut:
        run = engine.verify_chained_rlc if fast else engine.verify_chained
        res = run(first_round, bytes(prev0), [bytes(s) for s in sigs[:cut]])
        if res.first_bad is not None:
            return res.first_bad - first_round
    return None if cut == n else cut


class VerifyingClient:
    """Batched ``verifyingClient`` (client/verify.go:22-214) over one GPU engine.

    ``get(round) -> RandomData`` stands for ``indirectClient.Get``. ``chunk`` bounds how many rounds
    are fetched before one batched verify; the reference's order of errors is kept (a verify
    failure at round k is reported before a fetch failure at a later round).

    ``point_of_trust`` is ``WithVerifiedResult`` (client/client.go options; verify_test.go:19 seeds it
    with round 1). Reference quirk kept as is: without one, or for a round below it, the walk
    restarts at round 1 with ``GroupHash`` as the trusted signature (verify.go:131-137), so round 2
    is checked against ``Message(2, GroupHash)`` and rejects on a real chain.

    ``fast=True`` verifies the walked ranges with the randomized batch verification (see
    ``_verify_run``); the requested round itself is one beacon and always takes the exact check."""

    def __init__(self, engine, info: ChainInfo, get: Callable[[int], RandomData], strict=False,
                 v2from=UINT64_MAX, chunk=1 << 16, point_of_trust: Optional[RandomData] = None, fast=False):
        self.fast = bool(fast)
        self.engine = engine
        self.info = info
        self.get = get
        self.strict = strict
        self.v2from = v2from
        self.chunk = int(chunk)
        self.point_of_trust: Optional[RandomData] = point_of_trust
        self._pot_lk = threading.Lock()
        engine.set_public_key(info.public_key)

    def get_trusted_previous_signature(self, round_: int) -> bytes:
        """client/verify.go:115-174."""
        if round_ == 1:
            return self.info.group_hash
        with self._pot_lk:
            pot = self.point_of_trust
        if pot is None or pot.round > round_:
            trust_round, trust_prev = 1, self.get_trusted_previous_signature(1)
        else:
            trust_round, trust_prev = pot.round, pot.sig()
        initial = trust_round
        last_result = None
        while trust_round < round_ - 1:
            lo = trust_round + 1
            hi = min(round_ - 1, trust_round + self.chunk)
            results, fetch_err = [], None
            for r in range(lo, hi + 1):
                try:
                    results.append(self.get(r))
                except Exception as e:  # noqa: BLE001 - the reference wraps any client error
                    fetch_err = FetchError(r, e)
                    break
            sigs = [res.sig() for res in results]
            bad = _verify_run(self.engine, lo, trust_prev, sigs, self.fast)
            if bad is not None:
                raise VerifyError(lo + bad, f"verifying beacon: round {lo + bad}: bls: invalid signature")
            if fetch_err is not None:
                raise fetch_err
            trust_round = hi
            trust_prev = sigs[-1]
            last_result = results[-1]
        if trust_round == round_ - 1 and trust_round > initial:
            with self._pot_lk:
                self.point_of_trust = last_result
        if trust_round != round_ - 1:
            raise VerifyError(round_, f"unexpected trust round {trust_round}")
        return trust_prev

    def verify(self, r: RandomData) -> None:
        """client/verify.go:176-208: verify one result (V1 or V2) and set its randomness."""
        ps = r.previous_signature
        if r.round < self.v2from and (self.strict or r.previous_signature is None):
            ps = self.get_trusted_previous_signature(r.round)
        if r.round >= self.v2from:
            res = self.engine.verify_unchained([r.signature_v2], rounds=[r.round]) if len(r.signature_v2) == SIG_LEN \
                else None
            if res is None or not res.ok[0]:
                raise VerifyError(r.round, f"verification v2 of round {r.round} failed: bls: invalid signature")
            r.randomness = randomness_from_signature(r.signature_v2)
        else:
            bad = _verify_run(self.engine, r.round, ps, [r.signature])
            if bad is not None:
                raise VerifyError(r.round, f"verification v1 of round {r.round} failed: bls: invalid signature")
            r.randomness = randomness_from_signature(r.signature)


@dataclass
class SyncOutcome:
    """What ``syncer.tryNode`` (chain/beacon/sync.go:83-131) returns, plus why it stopped."""
    finished: bool            # the bool tryNode returns: last.Round == upTo was reached
    last: Beacon              # the store's last beacon afterwards
    stored: int               # beacons appended in this call
    reason: str = ""          # "", "invalid_beacon", "invalid round inserted", "invalid previous signature",
                              # "store", "stream ended"
    bad_round: Optional[int] = None


def sync_chain(engine, public_key: bytes, last: Beacon, packets: Iterable[Beacon], up_to: int,
               put: Callable[[Beacon], None], chunk=1 << 16, fast=False) -> SyncOutcome:
    """Batched ``syncer.tryNode`` + ``appendStore.Put`` over one GPU engine.

    Per chunk of the stream: the longest prefix that links (``Round == last.Round+1`` and
    ``PreviousSig == last.Signature``, store.go:43-48) is one chained range, verified in one call.
    Beacons are stored in order up to the first failure, exactly where the serial loop would stop
    (verify before Put, sync.go:105-113). The first unlinked beacon is verified on its own so the
    stop reason matches the reference's (a bad signature is reported before a linkage error).
    Unlike the serial loop, up to ``chunk`` packets are read from the stream ahead of the verify.
    ``fast=True`` verifies each linked range with the randomized batch verification (``_verify_run``)."""
    engine.set_public_key(public_key)
    stored = 0
    it = iter(packets)
    while True:
        batch = []
        for b in it:
            batch.append(b)
            if len(batch) >= chunk or b.round == up_to:
                break
        if not batch:
            return SyncOutcome(False, last, stored, "stream ended")
        # linked prefix
        linked, prev_r, prev_s = 0, last.round, last.signature
        for b in batch:
            if b.round != prev_r + 1 or bytes(b.previous_sig) != bytes(prev_s):
                break
            linked += 1
            prev_r, prev_s = b.round, b.signature
        bad = None
        if linked:
            bad = _verify_run(engine, batch[0].round, batch[0].previous_sig, [b.signature for b in batch[:linked]],
                              fast)
        ok_upto = linked if bad is None else bad
        for b in batch[:ok_upto]:
            try:
                put(b)
            except Exception:  # noqa: BLE001 - sync.go:110-113 logs and gives up on any store error
                return SyncOutcome(False, last, stored, "store", b.round)
            last = b
            stored += 1
            if last.round == up_to:
                return SyncOutcome(True, last, stored)
        if bad is not None:
            return SyncOutcome(False, last, stored, "invalid_beacon", batch[bad].round)
        if linked < len(batch):
            b = batch[linked]
            if _verify_run(engine, b.round, b.previous_sig, [b.signature]) is not None:
                return SyncOutcome(False, last, stored, "invalid_beacon", b.round)
            reason = "invalid round inserted" if b.round != last.round + 1 else "invalid previous signature"
            return SyncOutcome(False, last, stored, reason, b.round)


def verify_beacons(engine, public_key: bytes, beacons) -> list:
    """``chain.VerifyBeacon`` (chain/beacon.go:87-92) over an arbitrary list of beacons, e.g. a
    range loaded from a store or a relay: one ``verify_chained`` call per maximal linked run
    (``ingest.segments``). Returns one bool per beacon, in input order."""
    from .ingest import segments
    engine.set_public_key(public_key)
    ok = [False] * len(beacons)
    for seg in segments(beacons):
        if len(seg.sigs[0]) != SIG_LEN or len(seg.prev0) not in (32, 96):
            # a lone malformed beacon (wrong signature length) or an odd-length prev: one at a time
            for k, s in enumerate(seg.sigs):
                prev = seg.prev0 if k == 0 else seg.sigs[k - 1]
                ok[seg.start + k] = _verify_run(engine, seg.first_round + k, prev, [s]) is None
            continue
        res = engine.verify_chained(seg.first_round, seg.prev0, seg.sigs)
        ok[seg.start:seg.start + seg.n] = res.ok
    return ok


# --------------------------------------------------------------------------------------------------
# Timelock opening (core/timelock_test.go:43-60): the round's SignatureV2 is the IBE private key of
# everything encrypted to that round; timelock.Decrypt pairs each ciphertext's U with it, derives a key
# stream from the Gt value and XORs. Here all the ciphertexts of a round open in ONE engine call.

def kdf_sha256_ctr(gt: bytes, n: int) -> bytes:
    """This project's own example key-derivation: SHA-256(gt || BE32(counter)) blocks for counter =
    0, 1, ..., truncated to n bytes. It is NOT kyber's: the reference derives its key stream with
    BLAKE2Xs over ``GT.MarshalBinary``, which nothing in this repository can pin, so that KDF is not
    restated here. A deployment that must open the reference's ciphertexts passes its own ``kdf``."""
    out = b""
    counter = 0
    while len(out) < n:
        out += hashlib.sha256(bytes(gt) + counter.to_bytes(4, "big")).digest()
        counter += 1
    return out[:n]


def timelock_open(engine, round_: int, sig_v2: bytes, ciphertexts, kdf: Callable[[bytes, int], bytes],
                  verify: bool = True) -> list:
    """Opens every ciphertext locked to ``round_`` with that round's SignatureV2: ``ciphertexts`` is a
    sequence of ``(U48, C)`` (the ephemeral point rP, compressed, and the masked message); returns
    ``C XOR kdf(gt_i, len(C))`` per ciphertext with ``gt_i`` the 576-byte encoding of e(U_i, sig)^3
    (``Engine.tlock_open``), or ``None`` where U did not decode.

    ``verify=True`` first checks ``chain.VerifyBeaconV2`` of (round_, sig_v2) under the engine's group
    key (``verify_unchained``) and raises ``VerifyError`` on a reject: a wrong "private key" otherwise
    decrypts to silent garbage (the XXX of the reference's test). ``kdf(gt, n) -> n bytes`` is the
    caller's (see ``kdf_sha256_ctr``)."""
    sig_v2 = bytes(sig_v2)
    if verify:
        if len(sig_v2) != SIG_LEN:
            raise VerifyError(round_, "bad length")
        res = engine.verify_unchained([sig_v2], first_round=round_)
        if not res.ok[0]:
            from ._lib import REJ_NAMES
            raise VerifyError(round_, REJ_NAMES.get(res.reject_class[0], "bls: invalid signature"))
    cts = [(bytes(u), bytes(c)) for u, c in ciphertexts]
    good = [k for k, (u, _) in enumerate(cts) if len(u) == 48]  # a wrong length is rejected host-side
    res = engine.tlock_open(sig_v2, [cts[k][0] for k in good])
    gts = [None] * len(cts)
    for k, gt in zip(good, res.gt):
        gts[k] = gt
    out = []
    for (_, c), gt in zip(cts, gts):
        if gt is None:
            out.append(None)
            continue
        ks = kdf(gt, len(c))
        if len(ks) != len(c):
            raise ValueError("kdf returned %d bytes for a %d-byte ciphertext" % (len(ks), len(c)))
        out.append(bytes(a ^ b for a, b in zip(c, ks)))
    return out


def timelock_open_rounds(engine, rounds, kdf: Callable[[bytes, int], bytes], verify: bool = True) -> list:
    """Opens the ciphertexts of MANY rounds in ONE engine call (``Engine.tlock_open_rounds``): the shape
    of a vault back from downtime or an auditor opening a day of rounds. ``rounds`` is a sequence of
    ``(round, sig_v2, [(U48, C), ...])``; returns one list per round, each what
    ``timelock_open(engine, round, sig_v2, ciphertexts, kdf)`` gives: ``C XOR kdf(gt_i, len(C))`` per
    ciphertext, or ``None`` where U did not decode (a wrong-length U is filtered host-side).

    ``verify=True`` first checks all the signatures in one ``verify_unchained(sigs, rounds=...)`` under
    the engine's group key and raises ``VerifyError`` for the first rejected round before anything is
    opened. With ``verify=False`` a signature that does not even decode opens nothing: every ciphertext
    of its round is ``None``."""
    rounds = [(int(r), bytes(s), [(bytes(u), bytes(c)) for u, c in cts]) for r, s, cts in rounds]
    if verify:
        from ._lib import REJ_NAMES
        for r, s, _ in rounds:
            if len(s) != SIG_LEN:
                raise VerifyError(r, "bad length")
        if rounds:
            res = engine.verify_unchained([s for _, s, _ in rounds], rounds=[r for r, _, _ in rounds])
            for (r, _, _), ok, cls in zip(rounds, res.ok, res.reject_class):
                if not ok:
                    raise VerifyError(r, REJ_NAMES.get(cls, "bls: invalid signature"))
    good = [[k for k, (u, _) in enumerate(cts) if len(u) == 48] for _, _, cts in rounds]
    res = engine.tlock_open_rounds([s for _, s, _ in rounds],
                                   [[cts[k][0] for k in g] for (_, _, cts), g in zip(rounds, good)])
    out, at = [], 0
    for (_, _, cts), g in zip(rounds, good):
        gts = [None] * len(cts)
        for k in g:
            gts[k] = res.gt[at]
            at += 1
        opened = []
        for (_, c), gt in zip(cts, gts):
            if gt is None:
                opened.append(None)
                continue
            ks = kdf(gt, len(c))
            if len(ks) != len(c):
                raise ValueError("kdf returned %d bytes for a %d-byte ciphertext" % (len(ks), len(c)))
            opened.append(bytes(a ^ b for a, b in zip(c, ks)))
        out.append(opened)
    return out


def timelock_seal(engine, round_: int, messages, kdf: Callable[[bytes, int], bytes], scalars=None, pk48=None) -> list:
    """Locks every message to ``round_`` in ONE engine call (``Engine.tlock_seal``): returns a list of
    ``(U48, C)`` with ``U = k G1`` and ``C = m XOR kdf(gt, len(m))``, ``gt`` the 576-byte encoding of
    ``e(pk, H(MessageV2(round_)))^(3k)`` -- what ``timelock_open`` derives from U and the round's
    SignatureV2. ``pk48=None`` seals under the engine's group key.

    ``scalars=None`` draws one fresh secret scalar in [1, r) per message (``secrets.randbelow``). A
    caller who passes scalars owns their secrecy and uniqueness; one that is 0 mod r is refused by the
    engine and raises ``ValueError`` here. ``kdf`` is the caller's, as in ``timelock_open``."""
    msgs = [bytes(m) for m in messages]
    if scalars is None:
        import secrets
        from .engine import R_ORDER
        scalars = [secrets.randbelow(R_ORDER - 1) + 1 for _ in msgs]
    scalars = list(scalars)
    if len(scalars) != len(msgs):
        raise ValueError("%d scalars for %d messages" % (len(scalars), len(msgs)))
    res = engine.tlock_seal(round_, scalars, pk48=pk48)
    out = []
    for k, (m, ok, u, gt) in enumerate(zip(msgs, res.ok, res.us, res.gt)):
        if not ok:
            raise ValueError("scalar %d is 0 mod r: nothing can be sealed under it" % k)
        ks = kdf(gt, len(m))
        if len(ks) != len(m):
            raise ValueError("kdf returned %d bytes for a %d-byte message" % (len(ks), len(m)))
        out.append((u, bytes(a ^ b for a, b in zip(m, ks))))
    return out


def timelock_seal_rounds(engine, items, kdf: Callable[[bytes, int], bytes], scalars=None, pk48=None) -> list:
    """Locks every ``(round, message)`` of ``items`` to its OWN round in ONE engine call
    (``Engine.tlock_seal_rounds``): the shape of a sealing service, whose requests pick their unlock
    times themselves. Returns a list of ``(U48, C)`` in the order of ``items``, each what
    ``timelock_seal(engine, round, [message], ...)`` gives for its scalar; ``timelock_open`` with the
    round's SignatureV2 opens it. Scalars, ``kdf`` and ``pk48`` are as in ``timelock_seal``. Many
    messages for one round are better served by ``timelock_seal`` (no pairing per item)."""
    items = [(int(r), bytes(m)) for r, m in items]
    if scalars is None:
        import secrets
        from .engine import R_ORDER
        scalars = [secrets.randbelow(R_ORDER - 1) + 1 for _ in items]
    scalars = list(scalars)
    if len(scalars) != len(items):
        raise ValueError("%d scalars for %d messages" % (len(scalars), len(items)))
    res = engine.tlock_seal_rounds([r for r, _ in items], scalars, pk48=pk48)
    out = []
    for k, ((_, m), ok, u, gt) in enumerate(zip(items, res.ok, res.us, res.gt)):
        if not ok:
            raise ValueError("scalar %d is 0 mod r: nothing can be sealed under it" % k)
        ks = kdf(gt, len(m))
        if len(ks) != len(m):
            raise ValueError("kdf returned %d bytes for a %d-byte message" % (len(ks), len(m)))
        out.append((u, bytes(a ^ b for a, b in zip(m, ks))))
    return out


# Timelock in one call (include/blsverify.h "timelock in one call"): the four functions above under
# ``kdf_sha256_ctr`` with the key stream and the XOR done on the device, so that a call moves len(C) bytes
# per item instead of 576 and Python hashes nothing. The engine takes one message length per call: ragged
# lengths are padded with zeros to the call's longest and every result is cut back to its own length (the
# key stream is prefix-stable, so the bytes are those of the per-length result). A call with a message
# longer than ``TLOCK_MSG_MAX`` bytes or an empty one, or with nothing to do, goes through the function
# above with ``kdf_sha256_ctr``: the bytes are the same.

def _fused(lengths) -> int:
    """The padded length of a call the fused entry points take, or 0 for one that goes the long way."""
    from ._lib import TLOCK_MSG_MAX
    lengths = list(lengths)
    if not lengths or min(lengths) == 0 or max(lengths) > TLOCK_MSG_MAX:
        return 0
    return max(lengths)


def timelock_decrypt(engine, round_: int, sig_v2: bytes, ciphertexts, verify: bool = True) -> list:
    """``timelock_open(engine, round_, sig_v2, ciphertexts, kdf_sha256_ctr, verify)`` in one engine call
    (``Engine.tlock_decrypt``): the plaintext per ``(U48, C)``, or ``None`` where U did not decode (a
    wrong-length U is rejected host-side). ``verify`` is ``timelock_open``'s."""
    sig_v2 = bytes(sig_v2)
    cts = [(bytes(u), bytes(c)) for u, c in ciphertexts]
    good = [k for k, (u, _) in enumerate(cts) if len(u) == 48]
    mlen = _fused(len(cts[k][1]) for k in good)
    if not mlen:
        return timelock_open(engine, round_, sig_v2, cts, kdf_sha256_ctr, verify=verify)
    if verify:
        if len(sig_v2) != SIG_LEN:
            raise VerifyError(round_, "bad length")
        res = engine.verify_unchained([sig_v2], first_round=round_)
        if not res.ok[0]:
            from ._lib import REJ_NAMES
            raise VerifyError(round_, REJ_NAMES.get(res.reject_class[0], "bls: invalid signature"))
    res = engine.tlock_decrypt(sig_v2, [cts[k][0] for k in good], [cts[k][1].ljust(mlen, b"\0") for k in good])
    out = [None] * len(cts)
    for k, m in zip(good, res.msgs):
        out[k] = None if m is None else m[:len(cts[k][1])]
    return out


def timelock_decrypt_rounds(engine, rounds, verify: bool = True) -> list:
    """``timelock_open_rounds(engine, rounds, kdf_sha256_ctr, verify)`` in one engine call
    (``Engine.tlock_decrypt_rounds``): one list of plaintexts per ``(round, sig_v2, [(U48, C), ...])``."""
    rounds = [(int(r), bytes(s), [(bytes(u), bytes(c)) for u, c in cts]) for r, s, cts in rounds]
    good = [[k for k, (u, _) in enumerate(cts) if len(u) == 48] for _, _, cts in rounds]
    mlen = _fused(len(cts[k][1]) for (_, _, cts), g in zip(rounds, good) for k in g)
    if not mlen:
        return timelock_open_rounds(engine, rounds, kdf_sha256_ctr, verify=verify)
    if verify:
        from ._lib import REJ_NAMES
        for r, s, _ in rounds:
            if len(s) != SIG_LEN:
                raise VerifyError(r, "bad length")
        res = engine.verify_unchained([s for _, s, _ in rounds], rounds=[r for r, _, _ in rounds])
        for (r, _, _), ok, cls in zip(rounds, res.ok, res.reject_class):
            if not ok:
                raise VerifyError(r, REJ_NAMES.get(cls, "bls: invalid signature"))
    res = engine.tlock_decrypt_rounds([s for _, s, _ in rounds],
                                      [[cts[k][0] for k in g] for (_, _, cts), g in zip(rounds, good)],
                                      [[cts[k][1].ljust(mlen, b"\0") for k in g] for (_, _, cts), g in zip(rounds, good)])
    out, at = [], 0
    for (_, _, cts), g in zip(rounds, good):
        opened = [None] * len(cts)
        for k in g:
            m = res.msgs[at]
            at += 1
            opened[k] = None if m is None else m[:len(cts[k][1])]
        out.append(opened)
    return out


def timelock_encrypt(engine, round_: int, messages, scalars=None, pk48=None) -> list:
    """``timelock_seal(engine, round_, messages, kdf_sha256_ctr, scalars, pk48)`` in one engine call
    (``Engine.tlock_encrypt``): a list of ``(U48, C)``. The Gt values never reach the host."""
    msgs = [bytes(m) for m in messages]
    mlen = _fused(len(m) for m in msgs)
    if scalars is None:
        import secrets
        from .engine import R_ORDER
        scalars = [secrets.randbelow(R_ORDER - 1) + 1 for _ in msgs]
    scalars = list(scalars)
    if not mlen:
        return timelock_seal(engine, round_, msgs, kdf_sha256_ctr, scalars=scalars, pk48=pk48)
    if len(scalars) != len(msgs):
        raise ValueError("%d scalars for %d messages" % (len(scalars), len(msgs)))
    res = engine.tlock_encrypt(round_, scalars, [m.ljust(mlen, b"\0") for m in msgs], pk48=pk48)
    out = []
    for k, (m, ok, u, c) in enumerate(zip(msgs, res.ok, res.us, res.cs)):
        if not ok:
            raise ValueError("scalar %d is 0 mod r: nothing can be sealed under it" % k)
        out.append((u, c[:len(m)]))
    return out


def timelock_encrypt_rounds(engine, items, scalars=None, pk48=None) -> list:
    """``timelock_seal_rounds(engine, items, kdf_sha256_ctr, scalars, pk48)`` in one engine call
    (``Engine.tlock_encrypt_rounds``): a list of ``(U48, C)`` in the order of ``items``."""
    items = [(int(r), bytes(m)) for r, m in items]
    mlen = _fused(len(m) for _, m in items)
    if scalars is None:
        import secrets
        from .engine import R_ORDER
        scalars = [secrets.randbelow(R_ORDER - 1) + 1 for _ in items]
    scalars = list(scalars)
    if not mlen:
        return timelock_seal_rounds(engine, items, kdf_sha256_ctr, scalars=scalars, pk48=pk48)
    if len(scalars) != len(items):
        raise ValueError("%d scalars for %d messages" % (len(scalars), len(items)))
    res = engine.tlock_encrypt_rounds([r for r, _ in items], scalars, [m.ljust(mlen, b"\0") for _, m in items], pk48=pk48)
    out = []
    for k, ((_, m), ok, u, c) in enumerate(zip(items, res.ok, res.us, res.cs)):
        if not ok:
            raise ValueError("scalar %d is 0 mod r: nothing can be sealed under it" % k)
        out.append((u, c[:len(m)]))
    return out


# --------------------------------------------------------------------------------------------------
# Authenticated timelock (include/blsverify.h "authenticated timelock"): ciphertexts ``(U48, V32, W)`` that
# report whether they opened. The sealing scalar is H3(seed, message), so the message LENGTH enters the
# ciphertext: ragged inputs cannot be padded and cut back as above. They are grouped by length, one engine
# call per distinct length, and the results come back in input order. With ``ragged=True`` the whole input
# goes to the engine in ONE call instead (``Engine.tlock_*_auth*_var``: a length per item, blsverify.h "mixed
# message lengths in one call"), with the same results; the grouping stays the default. An empty message or one above
# ``TLOCK_MSG_MAX`` bytes raises ``ValueError``: there is no unfused function to fall back to.
# This is the project's own instantiation (SHA-256, its own tags and Gt encoding): NOT kyber's or tlock's.

def _auth_lengths(lengths):
    from ._lib import TLOCK_MSG_MAX
    for n in lengths:
        if not 1 <= n <= TLOCK_MSG_MAX:
            raise ValueError("an authenticated timelock message is 1 .. %d bytes, not %d" % (TLOCK_MSG_MAX, n))


def _by_length(lengths) -> dict:
    """{length: [indices]} in first-seen order."""
    groups: dict = {}
    for k, n in enumerate(lengths):
        groups.setdefault(n, []).append(k)
    return groups


def _auth_groups(lengths, ragged: bool) -> list:
    """The index lists of the engine calls: one per distinct length, or with ``ragged`` one for everything."""
    lengths = list(lengths)
    if ragged:
        return [list(range(len(lengths)))] if lengths else []
    return list(_by_length(lengths).values())


def _auth_seeds(seeds, n):
    if seeds is None:
        import secrets
        return [secrets.token_bytes(32) for _ in range(n)]
    seeds = [bytes(s) for s in seeds]
    if len(seeds) != n:
        raise ValueError("%d seeds for %d messages" % (len(seeds), n))
    return seeds


def _auth_verify(engine, pairs):
    from ._lib import REJ_NAMES
    for r, s in pairs:
        if len(s) != SIG_LEN:
            raise VerifyError(r, "bad length")
    res = engine.verify_unchained([s for _, s in pairs], rounds=[r for r, _ in pairs])
    for (r, _), ok, cls in zip(pairs, res.ok, res.reject_class):
        if not ok:
            raise VerifyError(r, REJ_NAMES.get(cls, "bls: invalid signature"))


def timelock_encrypt_auth(engine, round_: int, messages, seeds=None, pk48=None, ragged: bool = False) -> list:
    """A list of ``(U48, V32, W)``, message i locked to ``round_`` under pk48 (None = the group key) with
    ``seeds[i]`` -- 32 fresh bytes from ``secrets.token_bytes`` each when not given. One
    ``Engine.tlock_encrypt_auth`` call per distinct message length, or with ``ragged=True`` one
    ``Engine.tlock_encrypt_auth_var`` call for all of them."""
    msgs = [bytes(m) for m in messages]
    _auth_lengths(len(m) for m in msgs)
    seeds = _auth_seeds(seeds, len(msgs))
    out = [None] * len(msgs)
    call = engine.tlock_encrypt_auth_var if ragged else engine.tlock_encrypt_auth
    for idx in _auth_groups((len(m) for m in msgs), ragged):
        res = call(round_, [seeds[k] for k in idx], [msgs[k] for k in idx], pk48=pk48)
        for k, ok, u, v, w in zip(idx, res.ok, res.us, res.vs, res.ws):
            if not ok:
                raise ValueError("message %d: the derived scalar is 0 mod r; draw another seed" % k)
            out[k] = (u, v, w)
    return out


def timelock_encrypt_auth_rounds(engine, items, seeds=None, pk48=None, ragged: bool = False) -> list:
    """A list of ``(U48, V32, W)`` in the order of ``items`` = ``[(round, message), ...]``: one
    ``Engine.tlock_encrypt_auth_rounds`` call per distinct message length, or with ``ragged=True`` one
    ``Engine.tlock_encrypt_auth_rounds_var`` call for all of them."""
    items = [(int(r), bytes(m)) for r, m in items]
    _auth_lengths(len(m) for _, m in items)
    seeds = _auth_seeds(seeds, len(items))
    out = [None] * len(items)
    call = engine.tlock_encrypt_auth_rounds_var if ragged else engine.tlock_encrypt_auth_rounds
    for idx in _auth_groups((len(m) for _, m in items), ragged):
        res = call([items[k][0] for k in idx], [seeds[k] for k in idx], [items[k][1] for k in idx], pk48=pk48)
        for k, ok, u, v, w in zip(idx, res.ok, res.us, res.vs, res.ws):
            if not ok:
                raise ValueError("message %d: the derived scalar is 0 mod r; draw another seed" % k)
            out[k] = (u, v, w)
    return out


def _auth_openable(ct) -> bool:
    u, v, w = ct
    return len(u) == 48 and len(v) == 32


def timelock_decrypt_auth(engine, round_: int, sig_v2: bytes, ciphertexts, verify: bool = False,
                          ragged: bool = False) -> list:
    """The message per ``(U48, V32, W)``, or ``None`` for every item that did not authenticate or decode (a U or
    V of the wrong length is rejected host-side). ``verify`` defaults to **False** here: the ciphertext's own
    check subsumes the beacon verification -- under a signature that is not ``round_``'s every item fails it,
    so a wrong signature yields all ``None`` and no exception. ``verify=True`` runs ``verify_unchained`` first
    and raises ``VerifyError`` as ``timelock_decrypt`` does. One engine call per distinct W length, or with
    ``ragged=True`` one ``Engine.tlock_decrypt_auth_var`` call for every item that passed the host-side check."""
    sig_v2 = bytes(sig_v2)
    cts = [(bytes(u), bytes(v), bytes(w)) for u, v, w in ciphertexts]
    _auth_lengths(len(w) for _, _, w in cts)
    if verify:
        _auth_verify(engine, [(round_, sig_v2)])
    out = [None] * len(cts)
    good = [k for k, ct in enumerate(cts) if _auth_openable(ct)]
    call = engine.tlock_decrypt_auth_var if ragged else engine.tlock_decrypt_auth
    for idx in _auth_groups((len(cts[k][2]) for k in good), ragged):
        idx = [good[j] for j in idx]
        res = call(sig_v2, [cts[k][0] for k in idx], [cts[k][1] for k in idx], [cts[k][2] for k in idx])
        for k, m in zip(idx, res.msgs):
            out[k] = m
    return out


def timelock_decrypt_auth_rounds(engine, runs, verify: bool = False, ragged: bool = False) -> list:
    """One list of messages per ``(round, sig_v2, [(U48, V32, W), ...])``, ``None`` for every item that did not
    authenticate or decode (also every item of a round whose signature does not decode). ``verify`` as in
    ``timelock_decrypt_auth``. One ``Engine.tlock_decrypt_auth_rounds`` call per distinct W length, or with
    ``ragged=True`` one ``Engine.tlock_decrypt_auth_rounds_var`` call."""
    runs = [(int(r), bytes(s), [(bytes(u), bytes(v), bytes(w)) for u, v, w in cts]) for r, s, cts in runs]
    _auth_lengths(len(w) for _, _, cts in runs for _, _, w in cts)
    if verify:
        _auth_verify(engine, [(r, s) for r, s, _ in runs])
    out = [[None] * len(cts) for _, _, cts in runs]
    where = [(j, k) for j, (_, _, cts) in enumerate(runs) for k, ct in enumerate(cts) if _auth_openable(ct)]
    call = engine.tlock_decrypt_auth_rounds_var if ragged else engine.tlock_decrypt_auth_rounds
    for idx in _auth_groups((len(runs[j][2][k][2]) for j, k in where), ragged):
        picked = [where[i] for i in idx]
        per_round = [[k for jj, k in picked if jj == j] for j in range(len(runs))]
        res = call([s for _, s, _ in runs],
                   [[runs[j][2][k][0] for k in ks] for j, ks in enumerate(per_round)],
                   [[runs[j][2][k][1] for k in ks] for j, ks in enumerate(per_round)],
                   [[runs[j][2][k][2] for k in ks] for j, ks in enumerate(per_round)])
        at = 0
        for j, ks in enumerate(per_round):
            for k in ks:
                out[j][k] = res.msgs[at]
                at += 1
    return out


# --------------------------------------------------------------------------------------------------
# Threshold aggregation: chainStore.runAggregator (chain/beacon/chain.go:91-190)
# and its partialCache / roundCache (chain/beacon/cache.go:18-182), restated. The cache, the gate and
# the flush rules are host bookkeeping, as in the reference; the aggregation step itself (verify every
# cached V1 and V2 partial, Recover both, VerifyRecovered both) is ONE engine call,
# ``Engine.aggregate_round`` -> blsv_aggregate_round: two device passes for the whole round.

MAX_PARTIALS_PER_NODE = 100     # chain/beacon/constants.go:14
PARTIAL_CACHE_STORE_LIMIT = 3   # chain/beacon/chain.go:87

AGG_OK, AGG_OK_V2, AGG_V1_RECOVER_FAIL, AGG_V1_INVALID, AGG_V2_RECOVER_FAIL = range(5)  # include/blsverify.h


@dataclass
class PartialBeaconPacket:
    """``drand.PartialBeaconPacket`` (protobuf/drand/protocol.proto:62-72)."""
    round: int
    previous_sig: bytes
    partial_sig: bytes
    partial_sig_v2: bytes = b""


def index_of(partial: bytes) -> int:
    """``key.Scheme.IndexOf`` ([ext] tbls): the 2-byte big-endian share index; -1 on a short share
    (the callers ignore the error, cache.go:42,91,133)."""
    return int.from_bytes(bytes(partial[:2]), "big") if len(partial) >= 2 else -1


def message(round_: int, prev: bytes) -> bytes:
    """``chain.Message`` (chain/beacon.go:103-108)."""
    return hashlib.sha256(bytes(prev) + round_.to_bytes(8, "big")).digest()


def message_v2(round_: int) -> bytes:
    """``chain.MessageV2`` (chain/beacon.go:110-114)."""
    return hashlib.sha256(round_.to_bytes(8, "big")).digest()


class RoundCache:
    """``roundCache`` (cache.go:112-182): the partials of one (round, prev) keyed by share index."""

    def __init__(self, id_: bytes, p: PartialBeaconPacket):
        self.round = p.round
        self.prev = bytes(p.previous_sig)
        self.id = id_
        self.sigs: dict = {}
        self.sigs_v2: dict = {}

    def append(self, p: PartialBeaconPacket) -> bool:
        idx = index_of(p.partial_sig)
        if idx in self.sigs:
            return False
        self.sigs[idx] = bytes(p.partial_sig)
        if len(p.partial_sig_v2) > 0:  # a V2 partial missing the first time is never added later
            self.sigs_v2[idx] = bytes(p.partial_sig_v2)
        return True

    def __len__(self):
        return len(self.sigs)

    def len_v2(self):
        return len(self.sigs_v2)

    def msg(self):
        return message(self.round, self.prev)

    def partials(self):
        return list(self.sigs.values())

    def partials_v2(self):
        return list(self.sigs_v2.values())

    def flush_index(self, idx):
        self.sigs.pop(idx, None)


def round_id(round_: int, prev: bytes) -> bytes:
    """cache.go:33-38: BE64(round) || previous."""
    return round_.to_bytes(8, "big") + bytes(prev)


class PartialCache:
    """``partialCache`` (cache.go:18-110): per-round caches plus the per-signer round list that
    bounds a signer to MAX_PARTIALS_PER_NODE cached rounds (the oldest is evicted)."""

    def __init__(self, log=None):
        self.rounds: dict = {}
        self.rcvd: dict = {}
        self.log = log or (lambda *a: None)

    def append(self, p: PartialBeaconPacket):
        id_ = round_id(p.round, p.previous_sig)
        idx = index_of(p.partial_sig)
        rc = self._get_cache(id_, p)
        if rc is None:
            return
        if rc.append(p):
            self.rcvd.setdefault(idx, []).append(id_)

    def flush_rounds(self, round_: int):
        for id_, rc in list(self.rounds.items()):
            if rc.round > round_:
                continue
            del self.rounds[id_]
            for idx in list(rc.sigs):
                keep = [x for x in self.rcvd.get(idx, []) if x != id_]
                if keep:
                    self.rcvd[idx] = keep
                else:
                    self.rcvd.pop(idx, None)

    def get_round_cache(self, round_: int, prev: bytes):
        return self.rounds.get(round_id(round_, prev))

    def _get_cache(self, id_, p):
        if id_ in self.rounds:
            return self.rounds[id_]
        idx = index_of(p.partial_sig)
        if len(self.rcvd.get(idx, [])) >= MAX_PARTIALS_PER_NODE:
            to_evict = self.rcvd[idx][0]
            rc = self.rounds.get(to_evict)
            if rc is None:
                self.log("cache miss", idx, p.round)
                return None
            rc.flush_index(idx)
            self.rcvd[idx] = self.rcvd[idx][1:] + [id_]
            if len(rc) == 0:
                del self.rounds[to_evict]
        rc = RoundCache(id_, p)
        self.rounds[id_] = rc
        return rc


@dataclass
class AggregateEvent:
    """What one partial did to the aggregator (the reference only logs these)."""
    kind: str                       # "ignored", "stored", "invalid_recovery", "invalid_sig",
                                    # "invalid_recovery_v2", "aggregated"
    round: int
    beacon: Optional[Beacon] = None
    appended: bool = False          # tryAppend succeeded (chain.go:192-208)
    v2_valid: Optional[bool] = None  # VerifyRecovered V2 (a failure only logs, chain.go:162-164)


class Aggregator:
    """``chainStore.runAggregator`` (chain/beacon/chain.go:91-190) over one GPU engine.

    ``on_partial`` is the ``newPartials`` case (partials already passed ``ProcessPartialBeacon``'s
    VerifyPartial, node.go:112); ``on_beacon_stored`` the ``beaconStoredAgg`` case. ``put`` stands for
    ``CallbackStore.Put`` (raises on a rejected beacon). ``commits``/``t``/``n`` are the current
    group's (``c.crypto.GetPub()``, ``GetGroup().Threshold``/``Len()``); ``set_group`` follows a
    reshare transition (node.go:190)."""

    def __init__(self, engine, commits, t: int, n: int, last: Beacon, put: Callable[[Beacon], None]):
        self.engine = engine
        self.put = put
        self.last = last
        self.cache = PartialCache()
        self.set_group(commits, t, n)

    def set_group(self, commits, t, n):
        self.commits, self.t, self.n = [bytes(c) for c in commits], int(t), int(n)

    def on_beacon_stored(self, b: Beacon):
        self.last = b
        self.cache.flush_rounds(b.round)

    def on_partial(self, p: PartialBeaconPacket) -> AggregateEvent:
        r = p.round
        if not (self.last.round < r <= self.last.round + PARTIAL_CACHE_STORE_LIMIT + 1):
            return AggregateEvent("ignored", r)
        self.cache.append(p)
        rc = self.cache.get_round_cache(r, p.previous_sig)
        if rc is None or len(rc) < self.t:
            return AggregateEvent("stored", r)
        self.engine.set_group(self.commits, self.n)
        status, _, _, sig1, sig2, v2_valid = self.engine.aggregate_round(
            rc.msg(), rc.partials(), message_v2(r), rc.partials_v2(), self.t, self.n)
        if status == AGG_V1_RECOVER_FAIL:
            return AggregateEvent("invalid_recovery", r)
        if status == AGG_V1_INVALID:
            return AggregateEvent("invalid_sig", r)
        if status == AGG_V2_RECOVER_FAIL:
            return AggregateEvent("invalid_recovery_v2", r)
        b = Beacon(rc.prev, rc.round, sig1, sig2 if status == AGG_OK_V2 else b"")
        self.cache.flush_rounds(r)
        ev = AggregateEvent("aggregated", r, b, v2_valid=v2_valid if status == AGG_OK_V2 else None)
        if self.last.round + 1 == b.round:  # tryAppend (chain.go:192-208)
            try:
                self.put(b)
                ev.appended = True
                self.last = b
            except Exception:  # noqa: BLE001 - chain.go:197-200 logs and returns false
                pass
        return ev
