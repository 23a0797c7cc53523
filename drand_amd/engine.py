"""Python handle on one engine context (one HIP device, one stream): thin wrappers over the C ABI.

Every method runs the HIP kernels; nothing here computes a verdict on the CPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._lib import u8p, u32p, u64p


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"blsverify error {code}: {msg}")
        self.code = code


@dataclass
class BatchResult:
    """Outcome of a batch verify: ok[i] per item, first_bad (round or index, None if all ok),
    reject classes (REJ_*) per item."""
    ok: list
    first_bad: int | None
    reject_class: list

    @property
    def all_ok(self):
        return self.first_bad is None

    def bitmap(self):
        out = bytearray((len(self.ok) + 7) // 8)
        for i, v in enumerate(self.ok):
            if v:
                out[i // 8] |= 1 << (i % 8)
        return bytes(out)


class SignatureRejected(EngineError):
    """The shared signature of a timelock opening did not decode (sig_class = REJ_* 2-6)."""

    def __init__(self, code, msg, sig_class):
        super().__init__(code, msg)
        self.sig_class = sig_class


@dataclass
class TlockResult:
    """Outcome of Engine.tlock_open: ok[i] (U_i decoded), reject classes (REJ_*), gt[i] = the 576-byte
    encoding of e(U_i, sigma)^3 or None for a rejected U."""
    ok: list
    reject_class: list
    gt: list


@dataclass
class TlockRoundsResult:
    """Outcome of Engine.tlock_open_rounds: ok, reject_class and gt per item in packed order (as
    TlockResult's), sig_class[j] per round signature (0 = decoded)."""
    ok: list
    reject_class: list
    gt: list
    sig_class: list


# the order r of G1 / G2 / Gt: sealing scalars are taken mod r
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@dataclass
class TsealResult:
    """Outcome of Engine.tlock_seal: ok[i] (sealed), us[i] = compress(k_i G1), gt[i] = the 576-byte
    encoding of B^k_i; us[i] and gt[i] are None for a refused scalar (k_i == 0 mod r)."""
    ok: list
    us: list
    gt: list


@dataclass
class TdecryptResult:
    """Outcome of Engine.tlock_decrypt: ok[i] (U_i decoded), reject classes (REJ_*), msgs[i] = the item's mlen
    bytes cs[i] XOR kdf(e(U_i, sigma)^3), or None for a rejected item."""
    ok: list
    reject_class: list
    msgs: list


@dataclass
class TdecryptRoundsResult:
    """Outcome of Engine.tlock_decrypt_rounds: ok, reject_class and msgs per item in packed order (as
    TdecryptResult's), sig_class[j] per round signature (0 = decoded)."""
    ok: list
    reject_class: list
    msgs: list
    sig_class: list


@dataclass
class TencryptResult:
    """Outcome of Engine.tlock_encrypt: ok[i] (sealed), us[i] = compress(k_i G1), cs[i] = msgs[i] XOR kdf(K_i);
    us[i] and cs[i] are None for a refused scalar (k_i == 0 mod r). K_i itself never leaves the device."""
    ok: list
    us: list
    cs: list


@dataclass
class TencryptAuthResult:
    """Outcome of Engine.tlock_encrypt_auth: ok[i] (sealed), us[i] = compress(H3(seed_i, msg_i) G1), vs[i] the 32
    masked seed bytes, ws[i] the masked message; all three None for a refused item (a derived scalar == 0 mod r)."""
    ok: list
    us: list
    vs: list
    ws: list


@dataclass
class TdecryptAuthResult:
    """Outcome of Engine.tlock_decrypt_auth: ok[i] (the item decoded AND passed its re-encryption check), reject
    classes (REJ_*; REJ_TLOCK_AUTH for a failed check), msgs[i] = the message, or None where ok[i] is False."""
    ok: list
    reject_class: list
    msgs: list


@dataclass
class TdecryptAuthRoundsResult:
    """Outcome of Engine.tlock_decrypt_auth_rounds: ok, reject_class and msgs per item in packed order (as
    TdecryptAuthResult's), sig_class[j] per round signature (0 = decoded)."""
    ok: list
    reject_class: list
    msgs: list
    sig_class: list


def _packed(items, what):
    """Messages of one length 1 .. TLOCK_MSG_MAX, packed: (bytes, mlen)."""
    items = [bytes(x) for x in items]
    mlen = len(items[0]) if items else 1
    if any(len(x) != mlen for x in items):
        raise ValueError("%s of one call have one length (callers.timelock_* pads ragged ones)" % what)
    if not 1 <= mlen <= _lib.TLOCK_MSG_MAX:
        raise ValueError("%s are 1 .. %d bytes" % (what, _lib.TLOCK_MSG_MAX))
    return b"".join(items), mlen


def _scalar32(k):
    """A sealing scalar as 32 bytes big-endian: an int in [0, 2^256) or 32 bytes already."""
    if isinstance(k, (bytes, bytearray, memoryview)):
        k = bytes(k)
        if len(k) != 32:
            raise ValueError("scalars are 32 bytes big-endian")
        return k
    k = int(k)
    if not 0 <= k < 1 << 256:
        raise ValueError("scalars lie in [0, 2^256)")
    return k.to_bytes(32, "big")


def _bits(bitmap, n):
    import numpy as np
    if n == 0:
        return []
    return np.unpackbits(np.frombuffer(bytes(bitmap), np.uint8), bitorder="little")[:n].astype(bool).tolist()


class Engine:
    """One blsv_ctx. Not thread-safe (like the C context); create one per thread."""

    def __init__(self, device: int = 0, init_torch: bool = True):
        if init_torch:
            # torch ships its own HIP runtime next to /opt/rocm's. The order bench.py uses is the
            # one that works on the MI355X boxes: torch's runtime is up (a first allocation) before
            # libblsverify.so is loaded, and device buffers from torch are passed to the *_dev and
            # verify_prevs entry points.
            try:
                import torch
            except ImportError:
                torch = None
            if torch is not None:
                torch.cuda.set_device(int(device))
                torch.zeros(1, device=torch.device("cuda", int(device)))
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.blsv_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise EngineError(rc, f"blsv_create(device={device}) failed")
        self._h = h
        self._ops = None
        self.device = device

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.blsv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.blsv_last_error(self._h).decode())
        return rc

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        self._check(self.lib.blsv_synchronize(self._h))

    # ------------------------------------------------------------------ group
    def set_group(self, commits, n=None):
        """commits: list of 48-byte compressed G1 points (commits[0] = group public key)."""
        commits = [bytes(c) for c in commits]
        if any(len(c) != 48 for c in commits):
            raise ValueError("commitments must be 48 bytes")
        t = len(commits)
        self._check(self.lib.blsv_set_group(self._h, _lib.buf(b"".join(commits)), t, n if n is not None else t))

    def set_public_key(self, pk48):
        self.set_group([pk48], 1)

    # ------------------------------------------------------------------ verification
    def verify_chained(self, first_round, prev0, sigs):
        n = len(sigs)
        sigb = b"".join(bytes(s) for s in sigs)
        if any(len(s) != 96 for s in sigs):
            raise ValueError("chained signatures must be 96 bytes (reject wrong lengths host-side)")
        bm = _lib.out_buf((n + 7) // 8)
        fb = ctypes.c_uint64()
        cls = _lib.out_buf(n)
        self._check(self.lib.blsv_verify_chained(self._h, first_round, _lib.buf(prev0), len(prev0), _lib.buf(sigb), n,
                                                 bm, ctypes.byref(fb), cls))
        return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])

    def verify_chained_packed(self, first_round, prev0, sigs96, n):
        """``verify_chained`` over n signatures already packed as n*96 contiguous bytes (any object
        with the buffer protocol, e.g. a numpy slice of the bulk loader's SoA array)."""
        mv = memoryview(sigs96).cast("B")
        if len(mv) != 96 * n:
            raise ValueError("packed signatures must be n*96 bytes")
        bm = _lib.out_buf((n + 7) // 8)
        fb = ctypes.c_uint64()
        cls = _lib.out_buf(n)
        src = (ctypes.c_uint8 * max(len(mv), 1)).from_buffer_copy(mv) if len(mv) else None
        self._check(self.lib.blsv_verify_chained(self._h, first_round, _lib.buf(prev0), len(prev0), src, n, bm,
                                                 ctypes.byref(fb), cls))
        return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])

    def verify_prevs(self, first_round, prev0_len, prevs96, sigs96, n):
        """``chain.VerifyBeacon`` for n consecutive rounds, each with its own stored PreviousSig
        (``blsv_verify_prevs``): prevs96 / sigs96 are n*96 packed bytes (row 0's prev uses its first
        prev0_len = 32 or 96 bytes, every other row all 96). One device pass (drand.db ranges).
        Bulk form: ``ok`` and ``reject_class`` come back as numpy arrays, and the inputs are passed
        to the library without a host copy when they are contiguous numpy arrays."""
        import numpy as np
        p = np.ascontiguousarray(np.frombuffer(memoryview(prevs96).cast("B"), np.uint8))
        q = np.ascontiguousarray(np.frombuffer(memoryview(sigs96).cast("B"), np.uint8))
        if len(p) != 96 * n or len(q) != 96 * n:
            raise ValueError("prevs and sigs must be n*96 bytes")
        bm = np.zeros(max((n + 7) // 8, 1), np.uint8)
        cls = np.zeros(max(n, 1), np.uint8)
        fb = ctypes.c_uint64()
        u8 = ctypes.POINTER(ctypes.c_uint8)
        ptr = lambda a: a.ctypes.data_as(u8) if a.size else None
        self._check(self.lib.blsv_verify_prevs(self._h, first_round, ptr(p), prev0_len, ptr(q), n, ptr(bm),
                                               ctypes.byref(fb), ptr(cls)))
        ok = np.unpackbits(bm, bitorder="little")[:n].astype(bool)
        return BatchResult(ok, None if fb.value == 2 ** 64 - 1 else fb.value, cls[:n])

    def verify_unchained(self, sigs, first_round=None, rounds=None):
        n = len(sigs)
        if any(len(s) != 96 for s in sigs):
            raise ValueError("signatures must be 96 bytes (reject wrong lengths host-side)")
        sigb = b"".join(bytes(s) for s in sigs)
        rr = None
        if rounds is not None:
            rr = (ctypes.c_uint64 * max(n, 1))(*rounds)
        bm = _lib.out_buf((n + 7) // 8)
        fb = ctypes.c_uint64()
        cls = _lib.out_buf(n)
        self._check(self.lib.blsv_verify_unchained(self._h, rr, first_round or 0, _lib.buf(sigb), n, bm,
                                                   ctypes.byref(fb), cls))
        return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])

    def verify_messages(self, msgs, sigs, pk48=None):
        n = len(msgs)
        assert len(sigs) == n
        if any(len(s) != 96 for s in sigs):
            raise ValueError("signatures must be 96 bytes (reject wrong lengths host-side)")
        lens = (ctypes.c_uint32 * max(n, 1))(*[len(m) for m in msgs])
        bm = _lib.out_buf((n + 7) // 8)
        fb = ctypes.c_uint64()
        cls = _lib.out_buf(n)
        self._check(self.lib.blsv_verify_messages(self._h, _lib.buf(pk48) if pk48 is not None else None,
                                                  _lib.buf(b"".join(bytes(m) for m in msgs)), lens, n,
                                                  _lib.buf(b"".join(bytes(s) for s in sigs)), bm, ctypes.byref(fb),
                                                  cls))
        return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])

    def verify_partials(self, msg, partials):
        k = len(partials)
        plen = len(partials[0]) if k else 98
        if any(len(p) != plen for p in partials):
            raise ValueError("partials of one call must share a length")
        ok = _lib.out_buf(k)
        cls = _lib.out_buf(k)
        self._check(self.lib.blsv_verify_partials(self._h, _lib.buf(msg), len(msg),
                                                  _lib.buf(b"".join(bytes(p) for p in partials)), plen, k, ok, cls))
        return [bool(x) for x in list(ok)[:k]], list(cls)[:k]

    def verify_partials_multi(self, msgs, partials):
        """Partials of many rounds in one pass: partial i signs msgs[i] (blsv_verify_partials_multi)."""
        k = len(partials)
        assert len(msgs) == k
        plen = len(partials[0]) if k else 98
        if any(len(p) != plen for p in partials):
            raise ValueError("partials of one call must share a length")
        lens = (ctypes.c_uint32 * max(k, 1))(*[len(m) for m in msgs])
        ok = _lib.out_buf(k)
        cls = _lib.out_buf(k)
        self._check(self.lib.blsv_verify_partials_multi(self._h, _lib.buf(b"".join(bytes(m) for m in msgs)), lens,
                                                        _lib.buf(b"".join(bytes(p) for p in partials)), plen, k, ok,
                                                        cls))
        return [bool(x) for x in list(ok)[:k]], list(cls)[:k]

    def recover(self, msg, partials, t, n):
        k = len(partials)
        plen = len(partials[0]) if k else 98
        out = _lib.out_buf(96)
        self._check(self.lib.blsv_recover(self._h, _lib.buf(msg), len(msg),
                                          _lib.buf(b"".join(bytes(p) for p in partials)), plen, k, t, n, out))
        return bytes(out)

    def aggregate(self, msg, partials, t, n):
        """One aggregator round (blsv_aggregate): (ok per partial, reject classes, group sig, group_ok)."""
        k = len(partials)
        plen = len(partials[0]) if k else 98
        if any(len(p) != plen for p in partials):
            raise ValueError("partials of one call must share a length")
        ok = _lib.out_buf(k)
        cls = _lib.out_buf(k)
        out = _lib.out_buf(96)
        gok = _lib.out_buf(1)
        self._check(self.lib.blsv_aggregate(self._h, _lib.buf(msg), len(msg),
                                            _lib.buf(b"".join(bytes(p) for p in partials)), plen, k, t, n, ok, cls,
                                            out, gok))
        return [bool(x) for x in list(ok)[:k]], list(cls)[:k], bytes(out), bool(gok[0])

    def aggregate_round(self, msg1, partials1, msg2, partials2, t, n):
        """The aggregation step of one round cache, V1 + V2 (blsv_aggregate_round, chain.go:131-166):
        returns (status AGG_*, ok1, ok2, sig1, sig2 or None, v2_valid)."""
        # A share of the wrong length cannot parse: kyber's Recover skips it and VerifyPartial rejects
        # it, but it still counts in roundCache.Len()/LenV2() -- the V2 gate `LenV2() >= thr`
        # (chain.go:153) sees it. So it is passed on as a 98-byte share that can never verify (index
        # 0xFFFF >= n, compression flag clear): the C side counts it toward k2 >= t, rejects it
        # (ok = False at its position) and Recover skips it, exactly as kyber does.
        bad_share = b"\xff\xff" + bytes(96)
        partials1 = [p if len(p) == 98 else bad_share for p in (bytes(p) for p in partials1)]
        partials2 = [p if len(p) == 98 else bad_share for p in (bytes(p) for p in partials2)]
        k1, k2 = len(partials1), len(partials2)
        plen = 98
        ok1, ok2 = _lib.out_buf(k1), _lib.out_buf(k2)
        s1, s2 = _lib.out_buf(96), _lib.out_buf(96)
        st = ctypes.c_int32()
        v2 = _lib.out_buf(1)
        self._check(self.lib.blsv_aggregate_round(
            self._h, _lib.buf(msg1), len(msg1), _lib.buf(b"".join(partials1)), k1,
            _lib.buf(msg2), len(msg2), _lib.buf(b"".join(partials2)), k2, plen, t, n, ok1, ok2,
            s1, s2, ctypes.byref(st), v2))
        status = st.value
        sig1 = bytes(s1) if status in (_lib.AGG_OK, _lib.AGG_OK_V2, _lib.AGG_V1_INVALID,
                                       _lib.AGG_V2_RECOVER_FAIL) else None
        sig2 = bytes(s2) if status == _lib.AGG_OK_V2 else None
        r1 = [bool(x) for x in list(ok1)[:k1]]
        r2 = [bool(x) for x in list(ok2)[:k2]]
        return status, r1, r2, sig1, sig2, bool(v2[0])

    def sign(self, sk32, msgs, index=-1):
        n = len(msgs)
        lens = (ctypes.c_uint32 * max(n, 1))(*[len(m) for m in msgs])
        stride = 98 if index >= 0 else 96
        out = _lib.out_buf(n * stride)
        self._check(self.lib.blsv_sign(self._h, _lib.buf(sk32), index, _lib.buf(b"".join(bytes(m) for m in msgs)),
                                       lens, n, out))
        ob = bytes(out)
        return [ob[i * stride:(i + 1) * stride] for i in range(n)]

    def set_sign_lat_max(self, items):
        """blsv_set_sign_lat_max: sign calls of 1 .. items messages run on the latency path, one workgroup
        per message (0 = off, the default; clamped to the chunk); the outputs are byte for byte the batch
        path's. Returns the previous value."""
        return int(self.lib.blsv_set_sign_lat_max(self._h, int(items)))

    def sign_lat_stats(self):
        """(latency-path signing calls, messages they signed) since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_sign_lat_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ------------------------------------------------------------------ device-resident batches
    def verify_chained_dev(self, first_round, seg_len, d_seeds, seed0_len, d_sigs, n, d_bitmap, d_first_bad,
                           d_cls=None, stream=None, seg_phase=0):
        self._check(self.lib.blsv_verify_chained_dev(self._h, first_round, seg_len, seg_phase, d_seeds, seed0_len,
                                                     d_sigs, n, d_bitmap, d_first_bad, d_cls, stream))

    def generate_chained_dev(self, sk32, first_round, seg_len, d_seeds, seed0_len, d_sigs, n, stream=None):
        self._check(self.lib.blsv_generate_chained_dev(self._h, _lib.buf(sk32), first_round, seg_len, d_seeds,
                                                       seed0_len, d_sigs, n, stream))

    # ------------------------------------------------------------------ randomized batch verification
    # Opt-in (include/blsverify.h soundness contract): one pairing check per group of G beacons with
    # random 64-bit weights, the exact stages on every failing group. Same arguments and results as
    # the exact methods; a call with n <= lat_max or n < 2 G is served by the exact entry point.
    def verify_chained_rlc(self, first_round, prev0, sigs):
        n = len(sigs)
        if any(len(s) != 96 for s in sigs):
            raise ValueError("chained signatures must be 96 bytes (reject wrong lengths host-side)")
        sigb = b"".join(bytes(s) for s in sigs)
        bm = _lib.out_buf((n + 7) // 8)
        fb = ctypes.c_uint64()
        cls = _lib.out_buf(n)
        self._check(self.lib.blsv_verify_chained_rlc(self._h, first_round, _lib.buf(prev0), len(prev0), _lib.buf(sigb),
                                                     n, bm, ctypes.byref(fb), cls))
        return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])

    def verify_unchained_rlc(self, sigs, first_round=None, rounds=None):
        n = len(sigs)
        if any(len(s) != 96 for s in sigs):
            raise ValueError("signatures must be 96 bytes (reject wrong lengths host-side)")
        sigb = b"".join(bytes(s) for s in sigs)
        rr = None
        if rounds is not None:
            rr = (ctypes.c_uint64 * max(n, 1))(*rounds)
        bm = _lib.out_buf((n + 7) // 8)
        fb = ctypes.c_uint64()
        cls = _lib.out_buf(n)
        self._check(self.lib.blsv_verify_unchained_rlc(self._h, rr, first_round or 0, _lib.buf(sigb), n, bm,
                                                       ctypes.byref(fb), cls))
        return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])

    def verify_chained_rlc_dev(self, first_round, seg_len, d_seeds, seed0_len, d_sigs, n, d_bitmap, d_first_bad,
                               d_cls=None, stream=None, seg_phase=0):
        """As verify_chained_dev, but synchronises the stream once per pass (blsv_verify_chained_rlc_dev)."""
        self._check(self.lib.blsv_verify_chained_rlc_dev(self._h, first_round, seg_len, seg_phase, d_seeds, seed0_len,
                                                         d_sigs, n, d_bitmap, d_first_bad, d_cls, stream))

    def set_rlc_group(self, g):
        """Group size of the randomized path (a power of two in [8, 4096], default 64); returns the
        previous value."""
        return self.lib.blsv_set_rlc_group(self._h, int(g))

    def rlc_stats(self):
        """(group checks, failed group checks, items re-run exactly) since the context was created."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_rlc_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def test_rlc_seed(self, seed32):
        """Pin the randomized path's seed (32 bytes; None = a fresh seed per call again)."""
        if seed32 is not None and len(seed32) != 32:
            raise ValueError("the seed is 32 bytes")
        self._check(self.lib.blsv_test_rlc_seed(self._h, _lib.buf(seed32) if seed32 is not None else None))

    def test_rlc_sums(self, first_round, prev0, sigs):
        """blsv_test_rlc_sums: ([A_g], [B_g]) compressed, one pair per group of the chained range."""
        n = len(sigs)
        sigb = b"".join(bytes(s) for s in sigs)
        cap = -(-n // 8) + n // 16384 + 1  # the smallest group, one short group per pass of the smallest chunk
        a, b = _lib.out_buf(cap * 96), _lib.out_buf(cap * 96)
        ng = self.lib.blsv_test_rlc_sums(self._h, first_round, _lib.buf(prev0), len(prev0), _lib.buf(sigb), n, a, b)
        if ng < 0:
            raise EngineError(ng, self.lib.blsv_last_error(self._h).decode())
        ab, bb = bytes(a), bytes(b)
        return ([ab[96 * k:96 * k + 96] for k in range(ng)], [bb[96 * k:96 * k + 96] for k in range(ng)])

    # ------------------------------------------------------------------ timelock opening
    # include/blsverify.h "timelock": E_i = e(U_i, sigma)^3 for one shared round signature, 576 bytes
    # each (coefficient order and exponent as the header states them; parity with kilic unpinned).
    def tlock_open(self, sig, us):
        """blsv_tlock_open: TlockResult(ok, reject_class, gt) over the compressed G1 points `us` under
        the 96-byte round signature `sig`; gt[i] is 576 bytes, or None where U_i did not decode.
        Raises SignatureRejected (an EngineError, .sig_class = REJ_*) when sig does not decode. The
        signature is NOT verified here."""
        sig = bytes(sig)
        us = [bytes(u) for u in us]
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        if any(len(u) != 48 for u in us):
            raise ValueError("U values must be 48 bytes (reject wrong lengths host-side)")
        n = len(us)
        out = _lib.out_buf(n * 576)
        ok = _lib.out_buf(n)
        cls = _lib.out_buf(n)
        sc = ctypes.c_uint8()
        rc = self.lib.blsv_tlock_open(self._h, _lib.buf(sig), _lib.buf(b"".join(us)), n, out, ok, cls,
                                      ctypes.cast(ctypes.byref(sc), u8p))
        if rc == _lib.BLSV_EINVAL and sc.value:
            raise SignatureRejected(rc, self.lib.blsv_last_error(self._h).decode(), sc.value)
        self._check(rc)
        ob = bytes(out)
        oks = [bool(x) for x in list(ok)[:n]]
        return TlockResult(oks, list(cls)[:n], [ob[576 * i:576 * i + 576] if oks[i] else None for i in range(n)])

    def tlock_open_dev(self, sig, d_us, n, d_out, d_cls=None, stream=None):
        """blsv_tlock_open_dev: n device-resident U values (48 bytes each) -> n x 576 bytes at d_out
        (4-byte aligned), optional class bytes at d_cls; asynchronous on `stream` except for the
        read-back of a new signature's decode class."""
        sig = bytes(sig)
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        self._check(self.lib.blsv_tlock_open_dev(self._h, _lib.buf(sig), d_us, n, d_out, d_cls, stream))

    def tlock_stats(self):
        """(signatures prepared, U values processed) since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_tlock_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ------------------------------------------------------------------ timelock opening across many rounds
    # include/blsverify.h "timelock": m round signatures, round j owning a run of consecutive U values;
    # every item is what tlock_open(sigs[j], [U_i]) gives. Nothing is cached.
    @staticmethod
    def _rounds_args(sigs, counts):
        sigs = [bytes(s) for s in sigs]
        counts = [int(k) for k in counts]
        if any(len(s) != 96 for s in sigs):
            raise ValueError("a round signature is 96 bytes")
        if len(counts) != len(sigs) or any(not 0 <= k < 1 << 64 for k in counts):
            raise ValueError("one uint64 count per round signature")
        m = len(sigs)
        return _lib.buf(b"".join(sigs)), (ctypes.c_uint64 * max(m, 1))(*counts), m

    def tlock_open_rounds(self, sigs, us_per_round):
        """blsv_tlock_open_rounds: `sigs` are m 96-byte round signatures and `us_per_round` m sequences of
        compressed G1 points (round j's ciphertexts; an empty one is allowed). Returns
        TlockRoundsResult(ok, reject_class, gt, sig_class): ok, reject_class and gt in packed order (round
        0's items, then round 1's, ...), gt[i] 576 bytes or None where the item did not open; sig_class[j]
        = REJ_* of a signature that did not decode (its items have class REJ_TLOCK_SIG unless their own U
        is rejected) and 0 otherwise. The signatures are NOT verified here."""
        runs = [[bytes(u) for u in run] for run in us_per_round]
        us = [u for run in runs for u in run]
        if any(len(u) != 48 for u in us):
            raise ValueError("U values must be 48 bytes (reject wrong lengths host-side)")
        sb, counts, m = self._rounds_args(sigs, [len(run) for run in runs])
        n = len(us)
        out, ok, cls, sc = _lib.out_buf(n * 576), _lib.out_buf(n), _lib.out_buf(n), _lib.out_buf(m)
        self._check(self.lib.blsv_tlock_open_rounds(self._h, sb, counts, m, _lib.buf(b"".join(us)), n, out, ok, cls, sc))
        ob = bytes(out)
        oks = [bool(x) for x in list(ok)[:n]]
        return TlockRoundsResult(oks, list(cls)[:n], [ob[576 * i:576 * i + 576] if oks[i] else None for i in range(n)],
                                 list(sc)[:m])

    def tlock_open_rounds_dev(self, sigs, counts, d_us, n, d_out, d_cls=None, d_sig_cls=None, stream=None):
        """blsv_tlock_open_rounds_dev: `sigs` and `counts` (host: m signatures, m item counts summing to n)
        over n device-resident U values -> n x 576 bytes at d_out (4-byte aligned), optional class bytes at
        d_cls (n) and d_sig_cls (m); asynchronous on `stream`, no class is read back."""
        sb, cn, m = self._rounds_args(sigs, counts)
        self._check(self.lib.blsv_tlock_open_rounds_dev(self._h, sb, cn, m, d_us, n, d_out, d_cls, d_sig_cls, stream))

    def tlock_open_rounds_stats(self):
        """(signatures prepared, U values processed) by tlock_open_rounds* since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_tlock_open_rounds_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_tlock_dense_min(self, items):
        """blsv_set_tlock_dense_min: the shortest run that gets uniform tiles in tlock_open_rounds* (1 = every
        tile uniform, 2^64 - 1 = every tile mixed, 0 = the default); returns the previous value."""
        return int(self.lib.blsv_set_tlock_dense_min(self._h, int(items)))

    def set_tlock_lat_max(self, items):
        """blsv_set_tlock_lat_max: tlock_open / tlock_open_rounds calls of 1 .. items ciphertexts run on the
        latency path, one workgroup per ciphertext (0 = off, the default; clamped to the chunk); the outputs
        are byte for byte the batch path's. Returns the previous value."""
        return int(self.lib.blsv_set_tlock_lat_max(self._h, int(items)))

    def tlock_lat_stats(self):
        """(latency-path calls, U values they processed) since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_tlock_lat_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_tseal_lat_max(self, items):
        """blsv_set_tseal_lat_max: tlock_seal / tlock_seal_rounds calls of 1 .. items messages run on the
        latency path, one workgroup per message (0 = off, the default; clamped to the chunk); the outputs
        are byte for byte the batch path's. Returns the previous value."""
        return int(self.lib.blsv_set_tseal_lat_max(self._h, int(items)))

    def tseal_lat_stats(self):
        """(latency-path sealing calls, scalars they processed) since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_tseal_lat_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_tauth_lat_max(self, open_items=None, seal_items=None):
        """blsv_set_tauth_lat_max: tlock_decrypt_auth / _rounds calls of 1 .. open_items ciphertexts and
        tlock_encrypt_auth / _rounds calls of 1 .. seal_items messages run on the latency path of the
        authenticated forms, one workgroup per item (0 = off, the default; None = keep; clamped to the chunk);
        the outputs are byte for byte the batch path's. A switch of its own: set_tlock_lat_max and
        set_tseal_lat_max do not move these calls."""
        keep = ctypes.c_size_t(-1).value
        return int(self.lib.blsv_set_tauth_lat_max(self._h, keep if open_items is None else int(open_items),
                                                   keep if seal_items is None else int(seal_items)))

    def tauth_lat_stats(self):
        """(decrypting latency-path calls, ciphertexts they processed, encrypting latency-path calls, messages
        they processed) since the context was created."""
        v = [ctypes.c_uint64() for _ in range(4)]
        self._check(self.lib.blsv_tauth_lat_stats(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def test_tauth_walk_waves(self, waves):
        """blsv_test_tauth_walk_waves: 8 (the default) or 1 wave for the check's walk on that path."""
        self._check(self.lib.blsv_test_tauth_walk_waves(self._h, int(waves)))

    # ------------------------------------------------------------------ timelock sealing
    # include/blsverify.h "timelock": U_i = k_i G1 and K_i = B^k_i with B = e(pk, H(MessageV2(round)))^3
    # built once per (key, round); tlock_open(sigma_round, U_i) returns K_i.
    @staticmethod
    def _seal_key(pk48):
        if pk48 is None:
            return None
        pk48 = bytes(pk48)
        if len(pk48) != 48:
            raise ValueError("the public key is 48 bytes")
        return _lib.buf(pk48)

    def tlock_seal(self, round_, scalars, pk48=None):
        """blsv_tlock_seal: TsealResult(ok, us, gt) over `scalars` (ints below 2^256, or 32 bytes
        big-endian each; taken mod r) locked to `round_` under pk48 (None = the group key). A scalar
        == 0 (mod r) is refused: ok False, us and gt None. The scalars are the caller's secrets: draw them
        with `secrets`, fresh per item."""
        sc = [_scalar32(k) for k in scalars]
        n = len(sc)
        us, gt, ok = _lib.out_buf(n * 48), _lib.out_buf(n * 576), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_seal(self._h, self._seal_key(pk48), int(round_), _lib.buf(b"".join(sc)), n, us,
                                             gt, ok))
        ub, gb = bytes(us), bytes(gt)
        oks = [bool(x) for x in list(ok)[:n]]
        return TsealResult(oks, [ub[48 * i:48 * i + 48] if oks[i] else None for i in range(n)],
                           [gb[576 * i:576 * i + 576] if oks[i] else None for i in range(n)])

    def tlock_seal_dev(self, round_, d_scalars, n, d_us, d_gt, d_ok, pk48=None, stream=None):
        """blsv_tlock_seal_dev: n device-resident scalars (32 bytes each) -> n x 48 bytes at d_us, n x 576
        bytes at d_gt (4-byte aligned) and n ok bytes at d_ok; asynchronous on `stream` except for the
        build of a (key, round) that is not the cached one."""
        self._check(self.lib.blsv_tlock_seal_dev(self._h, self._seal_key(pk48), int(round_), d_scalars, n, d_us, d_gt,
                                                 d_ok, stream))

    def tlock_seal_stats(self):
        """(bases built, scalars processed) since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_tlock_seal_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ------------------------------------------------------------------ timelock sealing to many rounds
    # include/blsverify.h "timelock": item i locked to rounds[i]; its outputs are those of
    # tlock_seal(rounds[i], [scalars[i]]). One single-pair pairing per item, no base shared or cached.
    def tlock_seal_rounds(self, rounds, scalars, pk48=None):
        """blsv_tlock_seal_rounds: TsealResult(ok, us, gt), item i sealing scalars[i] (as tlock_seal takes
        them) to rounds[i] (any uint64) under pk48 (None = the group key). A scalar == 0 (mod r) is
        refused: ok False, us and gt None."""
        rounds = [int(r) for r in rounds]
        sc = [_scalar32(k) for k in scalars]
        n = len(sc)
        if len(rounds) != n:
            raise ValueError("%d rounds for %d scalars" % (len(rounds), n))
        if any(not 0 <= r < 1 << 64 for r in rounds):
            raise ValueError("a round is a uint64")
        us, gt, ok = _lib.out_buf(n * 48), _lib.out_buf(n * 576), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_seal_rounds(self._h, self._seal_key(pk48), (ctypes.c_uint64 * n)(*rounds),
                                                    _lib.buf(b"".join(sc)), n, us, gt, ok))
        ub, gb = bytes(us), bytes(gt)
        oks = [bool(x) for x in list(ok)[:n]]
        return TsealResult(oks, [ub[48 * i:48 * i + 48] if oks[i] else None for i in range(n)],
                           [gb[576 * i:576 * i + 576] if oks[i] else None for i in range(n)])

    def tlock_seal_rounds_dev(self, d_rounds, d_scalars, n, d_us, d_gt, d_ok, pk48=None, stream=None):
        """blsv_tlock_seal_rounds_dev: n device-resident rounds (uint64 each, 8-byte aligned) and scalars
        (32 bytes each) -> n x 48 bytes at d_us, n x 576 bytes at d_gt (4-byte aligned) and n ok bytes at
        d_ok; asynchronous on `stream` except for the decode of a key that is not the cached one."""
        self._check(self.lib.blsv_tlock_seal_rounds_dev(self._h, self._seal_key(pk48), d_rounds, d_scalars, n, d_us,
                                                        d_gt, d_ok, stream))

    def tlock_seal_rounds_stats(self):
        """(key tables built, scalars processed) since the context was created."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_tlock_seal_rounds_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ------------------------------------------------------------------ timelock in one call
    # include/blsverify.h "timelock in one call": the four passes above with the key stream (KDF_SHA256_CTR,
    # callers.kdf_sha256_ctr) and the XOR fused on the device; mlen bytes per item cross to the host, not 576.
    def tlock_decrypt(self, sig, us, cs, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt: TdecryptResult(ok, reject_class, msgs) over the ciphertexts (us[i], cs[i]) under
        the 96-byte round signature `sig`; every cs[i] has the same length, 1 .. 256 bytes. msgs[i] equals
        cs[i] XOR kdf_sha256_ctr(tlock_open(sig, us).gt[i]), or None where U_i did not decode. Raises
        SignatureRejected as tlock_open does. The signature is NOT verified here."""
        sig = bytes(sig)
        us = [bytes(u) for u in us]
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        if any(len(u) != 48 for u in us):
            raise ValueError("U values must be 48 bytes (reject wrong lengths host-side)")
        n = len(us)
        cb, mlen = _packed(cs, "ciphertexts")
        if len(cb) != n * mlen:
            raise ValueError("one ciphertext per U value")
        out, ok, cls = _lib.out_buf(n * mlen), _lib.out_buf(n), _lib.out_buf(n)
        sc = ctypes.c_uint8()
        rc = self.lib.blsv_tlock_decrypt(self._h, _lib.buf(sig), _lib.buf(b"".join(us)), _lib.buf(cb), mlen, n, int(kdf),
                                         out, ok, cls, ctypes.cast(ctypes.byref(sc), u8p))
        if rc == _lib.BLSV_EINVAL and sc.value:
            raise SignatureRejected(rc, self.lib.blsv_last_error(self._h).decode(), sc.value)
        self._check(rc)
        ob = bytes(out)
        oks = [bool(x) for x in list(ok)[:n]]
        return TdecryptResult(oks, list(cls)[:n], [ob[mlen * i:mlen * i + mlen] if oks[i] else None for i in range(n)])

    def tlock_decrypt_dev(self, sig, d_us, d_cs, mlen, n, d_out, d_cls=None, stream=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_dev: n device-resident U values (48 bytes each) and ciphertexts (mlen bytes each,
        any alignment) -> n x mlen bytes at d_out (d_out == d_cs is allowed), optional class bytes at d_cls;
        asynchronous on `stream` except for the read-back of a new signature's decode class."""
        sig = bytes(sig)
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        self._check(self.lib.blsv_tlock_decrypt_dev(self._h, _lib.buf(sig), d_us, d_cs, int(mlen), n, int(kdf), d_out,
                                                    d_cls, stream))

    def tlock_decrypt_rounds(self, sigs, us_per_round, cs_per_round, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_rounds: as tlock_open_rounds takes `sigs` and `us_per_round`, with round j's
        ciphertext bodies in cs_per_round[j] (one length for the whole call). Returns
        TdecryptRoundsResult(ok, reject_class, msgs, sig_class) in packed order; msgs[i] is None where the
        item did not open. The signatures are NOT verified here."""
        runs = [[bytes(u) for u in run] for run in us_per_round]
        us = [u for run in runs for u in run]
        if any(len(u) != 48 for u in us):
            raise ValueError("U values must be 48 bytes (reject wrong lengths host-side)")
        cruns = [list(run) for run in cs_per_round]
        if [len(r) for r in cruns] != [len(r) for r in runs]:
            raise ValueError("one ciphertext per U value, round by round")
        sb, counts, m = self._rounds_args(sigs, [len(run) for run in runs])
        n = len(us)
        cb, mlen = _packed([c for run in cruns for c in run], "ciphertexts")
        out, ok, cls, sc = _lib.out_buf(n * mlen), _lib.out_buf(n), _lib.out_buf(n), _lib.out_buf(m)
        self._check(self.lib.blsv_tlock_decrypt_rounds(self._h, sb, counts, m, _lib.buf(b"".join(us)), _lib.buf(cb), mlen,
                                                       n, int(kdf), out, ok, cls, sc))
        ob = bytes(out)
        oks = [bool(x) for x in list(ok)[:n]]
        return TdecryptRoundsResult(oks, list(cls)[:n],
                                    [ob[mlen * i:mlen * i + mlen] if oks[i] else None for i in range(n)], list(sc)[:m])

    def tlock_decrypt_rounds_dev(self, sigs, counts, d_us, d_cs, mlen, n, d_out, d_cls=None, d_sig_cls=None, stream=None,
                                 kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_rounds_dev: `sigs` and `counts` on the host over n device-resident U values and
        ciphertexts (mlen bytes each, any alignment) -> n x mlen bytes at d_out, optional class bytes at d_cls
        (n) and d_sig_cls (m); asynchronous on `stream`, no class is read back."""
        sb, cn, m = self._rounds_args(sigs, counts)
        self._check(self.lib.blsv_tlock_decrypt_rounds_dev(self._h, sb, cn, m, d_us, d_cs, int(mlen), n, int(kdf), d_out,
                                                           d_cls, d_sig_cls, stream))

    def _encrypt_result(self, n, mlen, us, cs, ok):
        ub, cb = bytes(us), bytes(cs)
        oks = [bool(x) for x in list(ok)[:n]]
        return TencryptResult(oks, [ub[48 * i:48 * i + 48] if oks[i] else None for i in range(n)],
                              [cb[mlen * i:mlen * i + mlen] if oks[i] else None for i in range(n)])

    def tlock_encrypt(self, round_, scalars, msgs, pk48=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt: TencryptResult(ok, us, cs), message i (one length per call, 1 .. 256 bytes)
        locked to `round_` with scalars[i] (as tlock_seal takes them) under pk48 (None = the group key):
        cs[i] = msgs[i] XOR kdf_sha256_ctr(K_i) with K_i what tlock_seal returns as gt[i]. A scalar == 0
        (mod r) is refused: ok False, us and cs None."""
        sc = [_scalar32(k) for k in scalars]
        n = len(sc)
        mb, mlen = _packed(msgs, "messages")
        if len(mb) != n * mlen:
            raise ValueError("one message per scalar")
        us, cs, ok = _lib.out_buf(n * 48), _lib.out_buf(n * mlen), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_encrypt(self._h, self._seal_key(pk48), int(round_), _lib.buf(b"".join(sc)),
                                                _lib.buf(mb), mlen, n, int(kdf), us, cs, ok))
        return self._encrypt_result(n, mlen, us, cs, ok)

    def tlock_encrypt_dev(self, round_, d_scalars, d_msgs, mlen, n, d_us, d_cs, d_ok, pk48=None, stream=None,
                          kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_dev: n device-resident scalars (32 bytes each) and messages (mlen bytes each, any
        alignment) -> n x 48 bytes at d_us, n x mlen bytes at d_cs (d_cs == d_msgs is allowed) and n ok bytes
        at d_ok; asynchronous on `stream` except for the build of a (key, round) that is not the cached one."""
        self._check(self.lib.blsv_tlock_encrypt_dev(self._h, self._seal_key(pk48), int(round_), d_scalars, d_msgs,
                                                    int(mlen), n, int(kdf), d_us, d_cs, d_ok, stream))

    def tlock_encrypt_rounds(self, rounds, scalars, msgs, pk48=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_rounds: TencryptResult(ok, us, cs), message i locked to rounds[i] (any uint64) with
        scalars[i]; the outputs are those of tlock_encrypt(rounds[i], [scalars[i]], [msgs[i]])."""
        rounds = [int(r) for r in rounds]
        sc = [_scalar32(k) for k in scalars]
        n = len(sc)
        if len(rounds) != n:
            raise ValueError("%d rounds for %d scalars" % (len(rounds), n))
        if any(not 0 <= r < 1 << 64 for r in rounds):
            raise ValueError("a round is a uint64")
        mb, mlen = _packed(msgs, "messages")
        if len(mb) != n * mlen:
            raise ValueError("one message per scalar")
        us, cs, ok = _lib.out_buf(n * 48), _lib.out_buf(n * mlen), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_encrypt_rounds(self._h, self._seal_key(pk48), (ctypes.c_uint64 * max(n, 1))(*rounds),
                                                       _lib.buf(b"".join(sc)), _lib.buf(mb), mlen, n, int(kdf), us, cs, ok))
        return self._encrypt_result(n, mlen, us, cs, ok)

    def tlock_encrypt_rounds_dev(self, d_rounds, d_scalars, d_msgs, mlen, n, d_us, d_cs, d_ok, pk48=None, stream=None,
                                 kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_rounds_dev: n device-resident rounds (uint64 each, 8-byte aligned), scalars and
        messages (mlen bytes each, any alignment) -> d_us, d_cs and d_ok as tlock_encrypt_dev writes them."""
        self._check(self.lib.blsv_tlock_encrypt_rounds_dev(self._h, self._seal_key(pk48), d_rounds, d_scalars, d_msgs,
                                                           int(mlen), n, int(kdf), d_us, d_cs, d_ok, stream))

    # ------------------------------------------------------------------ authenticated timelock
    # include/blsverify.h "authenticated timelock": the Fujisaki-Okamoto transform over the passes above. A
    # ciphertext is (U, V, W); the sealing scalar is H3(seed, msg); a decrypt reports per item whether the
    # ciphertext opened (REJ_TLOCK_AUTH otherwise). The project's own instantiation: not kyber's, not tlock's.
    @staticmethod
    def _rows(items, size, what):
        items = [bytes(x) for x in items]
        if any(len(x) != size for x in items):
            raise ValueError("%s are %d bytes" % (what, size))
        return items

    def _encrypt_auth_result(self, n, mlen, us, vs, ws, ok):
        ub, vb, wb = bytes(us), bytes(vs), bytes(ws)
        oks = [bool(x) for x in list(ok)[:n]]
        return TencryptAuthResult(oks, [ub[48 * i:48 * i + 48] if oks[i] else None for i in range(n)],
                                  [vb[32 * i:32 * i + 32] if oks[i] else None for i in range(n)],
                                  [wb[mlen * i:mlen * i + mlen] if oks[i] else None for i in range(n)])

    def tlock_encrypt_auth(self, round_, seeds, msgs, pk48=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_auth: TencryptAuthResult(ok, us, vs, ws), message i (one length per call, 1 .. 256
        bytes) locked to `round_` under pk48 (None = the group key) with the 32-byte seed seeds[i], which the
        CALLER draws fresh and at random per item (callers.timelock_encrypt_auth does)."""
        sd = self._rows(seeds, _lib.SEED_LEN, "seeds")
        n = len(sd)
        mb, mlen = _packed(msgs, "messages")
        if len(mb) != n * mlen:
            raise ValueError("one message per seed")
        us, vs, ws, ok = _lib.out_buf(n * 48), _lib.out_buf(n * 32), _lib.out_buf(n * mlen), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_encrypt_auth(self._h, self._seal_key(pk48), int(round_), _lib.buf(b"".join(sd)),
                                                     _lib.buf(mb), mlen, n, int(kdf), us, vs, ws, ok))
        return self._encrypt_auth_result(n, mlen, us, vs, ws, ok)

    def tlock_encrypt_auth_dev(self, round_, d_seeds, d_msgs, mlen, n, d_us, d_vs, d_ws, d_ok, pk48=None, stream=None,
                               kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_auth_dev: n device-resident seeds (32 bytes each) and messages (mlen bytes each, any
        alignment) -> n x 48 bytes at d_us, n x 32 at d_vs, n x mlen at d_ws (d_ws == d_msgs is allowed) and n ok
        bytes at d_ok; asynchronous on `stream` except for the build of a (key, round) that is not the cached one."""
        self._check(self.lib.blsv_tlock_encrypt_auth_dev(self._h, self._seal_key(pk48), int(round_), d_seeds, d_msgs,
                                                         int(mlen), n, int(kdf), d_us, d_vs, d_ws, d_ok, stream))

    def tlock_encrypt_auth_rounds(self, rounds, seeds, msgs, pk48=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_auth_rounds: TencryptAuthResult, message i locked to rounds[i] (any uint64) with
        seeds[i]; the outputs are those of tlock_encrypt_auth(rounds[i], [seeds[i]], [msgs[i]])."""
        rounds = [int(r) for r in rounds]
        sd = self._rows(seeds, _lib.SEED_LEN, "seeds")
        n = len(sd)
        if len(rounds) != n:
            raise ValueError("%d rounds for %d seeds" % (len(rounds), n))
        if any(not 0 <= r < 1 << 64 for r in rounds):
            raise ValueError("a round is a uint64")
        mb, mlen = _packed(msgs, "messages")
        if len(mb) != n * mlen:
            raise ValueError("one message per seed")
        us, vs, ws, ok = _lib.out_buf(n * 48), _lib.out_buf(n * 32), _lib.out_buf(n * mlen), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_encrypt_auth_rounds(self._h, self._seal_key(pk48),
                                                            (ctypes.c_uint64 * max(n, 1))(*rounds), _lib.buf(b"".join(sd)),
                                                            _lib.buf(mb), mlen, n, int(kdf), us, vs, ws, ok))
        return self._encrypt_auth_result(n, mlen, us, vs, ws, ok)

    def tlock_encrypt_auth_rounds_dev(self, d_rounds, d_seeds, d_msgs, mlen, n, d_us, d_vs, d_ws, d_ok, pk48=None,
                                      stream=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_auth_rounds_dev: n device-resident rounds (uint64 each, 8-byte aligned), seeds and
        messages -> d_us, d_vs, d_ws and d_ok as tlock_encrypt_auth_dev writes them."""
        self._check(self.lib.blsv_tlock_encrypt_auth_rounds_dev(self._h, self._seal_key(pk48), d_rounds, d_seeds, d_msgs,
                                                                int(mlen), n, int(kdf), d_us, d_vs, d_ws, d_ok, stream))

    def tlock_decrypt_auth(self, sig, us, vs, ws, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_auth: TdecryptAuthResult(ok, reject_class, msgs) over the ciphertexts (us[i], vs[i],
        ws[i]) under the 96-byte round signature `sig`; every ws[i] has the same length, 1 .. 256 bytes. msgs[i]
        is the message where the item decoded and passed its check, else None (REJ_TLOCK_AUTH, or U's decode
        class). Raises SignatureRejected as tlock_open does for a signature that does not decode. No beacon
        verification is needed beside it: under a signature of another round every item is REJ_TLOCK_AUTH."""
        sig = bytes(sig)
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        us = self._rows(us, 48, "U values")
        vs = self._rows(vs, _lib.V_LEN, "V values")
        n = len(us)
        wb, mlen = _packed(ws, "ciphertexts")
        if len(wb) != n * mlen or len(vs) != n:
            raise ValueError("one V and one W per U value")
        out, ok, cls = _lib.out_buf(n * mlen), _lib.out_buf(n), _lib.out_buf(n)
        sc = ctypes.c_uint8()
        rc = self.lib.blsv_tlock_decrypt_auth(self._h, _lib.buf(sig), _lib.buf(b"".join(us)), _lib.buf(b"".join(vs)),
                                              _lib.buf(wb), mlen, n, int(kdf), out, ok, cls,
                                              ctypes.cast(ctypes.byref(sc), u8p))
        if rc == _lib.BLSV_EINVAL and sc.value:
            raise SignatureRejected(rc, self.lib.blsv_last_error(self._h).decode(), sc.value)
        self._check(rc)
        ob = bytes(out)
        oks = [bool(x) for x in list(ok)[:n]]
        return TdecryptAuthResult(oks, list(cls)[:n], [ob[mlen * i:mlen * i + mlen] if oks[i] else None for i in range(n)])

    def tlock_decrypt_auth_dev(self, sig, d_us, d_vs, d_ws, mlen, n, d_out, d_cls, stream=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_auth_dev: n device-resident ciphertexts -> n x mlen bytes at d_out (d_out == d_ws is
        allowed; zeros for an item that is not good) and the class bytes at d_cls, which is REQUIRED; asynchronous
        on `stream` except for the read-back of a new signature's decode class."""
        sig = bytes(sig)
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        self._check(self.lib.blsv_tlock_decrypt_auth_dev(self._h, _lib.buf(sig), d_us, d_vs, d_ws, int(mlen), n, int(kdf),
                                                         d_out, d_cls, stream))

    def tlock_decrypt_auth_rounds(self, sigs, us_per_round, vs_per_round, ws_per_round, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_auth_rounds: as tlock_decrypt_rounds takes `sigs` and `us_per_round`, with round j's V
        and W values in vs_per_round[j] / ws_per_round[j] (one W length for the whole call). Returns
        TdecryptAuthRoundsResult(ok, reject_class, msgs, sig_class) in packed order."""
        runs = [self._rows(run, 48, "U values") for run in us_per_round]
        vruns = [self._rows(run, _lib.V_LEN, "V values") for run in vs_per_round]
        wruns = [list(run) for run in ws_per_round]
        if [len(r) for r in vruns] != [len(r) for r in runs] or [len(r) for r in wruns] != [len(r) for r in runs]:
            raise ValueError("one V and one W per U value, round by round")
        us = [u for run in runs for u in run]
        sb, counts, m = self._rounds_args(sigs, [len(run) for run in runs])
        n = len(us)
        wb, mlen = _packed([w for run in wruns for w in run], "ciphertexts")
        out, ok, cls, sc = _lib.out_buf(n * mlen), _lib.out_buf(n), _lib.out_buf(n), _lib.out_buf(m)
        self._check(self.lib.blsv_tlock_decrypt_auth_rounds(self._h, sb, counts, m, _lib.buf(b"".join(us)),
                                                            _lib.buf(b"".join(v for run in vruns for v in run)),
                                                            _lib.buf(wb), mlen, n, int(kdf), out, ok, cls, sc))
        ob = bytes(out)
        oks = [bool(x) for x in list(ok)[:n]]
        return TdecryptAuthRoundsResult(oks, list(cls)[:n],
                                        [ob[mlen * i:mlen * i + mlen] if oks[i] else None for i in range(n)],
                                        list(sc)[:m])

    def tlock_decrypt_auth_rounds_dev(self, sigs, counts, d_us, d_vs, d_ws, mlen, n, d_out, d_cls, d_sig_cls=None,
                                      stream=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_auth_rounds_dev: `sigs` and `counts` on the host over n device-resident ciphertexts
        -> n x mlen bytes at d_out, the class bytes at d_cls (REQUIRED, n) and optionally d_sig_cls (m);
        asynchronous on `stream`, no class is read back."""
        sb, cn, m = self._rounds_args(sigs, counts)
        self._check(self.lib.blsv_tlock_decrypt_auth_rounds_dev(self._h, sb, cn, m, d_us, d_vs, d_ws, int(mlen), n,
                                                                int(kdf), d_out, d_cls, d_sig_cls, stream))

    # ---- mixed message lengths in one call (include/blsverify.h "mixed message lengths in one call"): the four
    # host forms above with a length per item. The length enters H3, so nothing here pads: the bytes travel packed
    # back to back with their lengths beside them, and every result is cut at its own length.
    @staticmethod
    def _ragged(items, what):
        items = [bytes(x) for x in items]
        lens = [len(x) for x in items]
        if any(v >= 1 << 32 for v in lens):
            raise ValueError("%s: a length is a uint32" % what)
        return b"".join(items), lens, (ctypes.c_uint32 * max(len(lens), 1))(*lens)

    @staticmethod
    def _cut(buf, lens, oks):
        b, out, at = bytes(buf), [], 0
        for v, good in zip(lens, oks):
            out.append(b[at:at + v] if good else None)
            at += v
        return out

    def _encrypt_auth_var_result(self, n, lens, us, vs, ws, ok):
        ub, vb = bytes(us), bytes(vs)
        oks = [bool(x) for x in list(ok)[:n]]
        return TencryptAuthResult(oks, [ub[48 * i:48 * i + 48] if oks[i] else None for i in range(n)],
                                  [vb[32 * i:32 * i + 32] if oks[i] else None for i in range(n)], self._cut(ws, lens, oks))

    def tlock_encrypt_auth_var(self, round_, seeds, msgs, pk48=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_auth_var: tlock_encrypt_auth over messages of ANY lengths (1 .. 256 bytes each) in one
        call; item i's (U, V, W) are what tlock_encrypt_auth gives for it in a call of its own length."""
        sd = self._rows(seeds, _lib.SEED_LEN, "seeds")
        n = len(sd)
        mb, lens, cl = self._ragged(msgs, "messages")
        if len(lens) != n:
            raise ValueError("one message per seed")
        us, vs, ws, ok = _lib.out_buf(n * 48), _lib.out_buf(n * 32), _lib.out_buf(len(mb)), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_encrypt_auth_var(self._h, self._seal_key(pk48), int(round_), _lib.buf(b"".join(sd)),
                                                         _lib.buf(mb), cl, n, int(kdf), us, vs, ws, ok))
        return self._encrypt_auth_var_result(n, lens, us, vs, ws, ok)

    def tlock_encrypt_auth_rounds_var(self, rounds, seeds, msgs, pk48=None, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_encrypt_auth_rounds_var: tlock_encrypt_auth_rounds over messages of any lengths in one call."""
        rounds = [int(r) for r in rounds]
        sd = self._rows(seeds, _lib.SEED_LEN, "seeds")
        n = len(sd)
        if len(rounds) != n:
            raise ValueError("%d rounds for %d seeds" % (len(rounds), n))
        if any(not 0 <= r < 1 << 64 for r in rounds):
            raise ValueError("a round is a uint64")
        mb, lens, cl = self._ragged(msgs, "messages")
        if len(lens) != n:
            raise ValueError("one message per seed")
        us, vs, ws, ok = _lib.out_buf(n * 48), _lib.out_buf(n * 32), _lib.out_buf(len(mb)), _lib.out_buf(n)
        self._check(self.lib.blsv_tlock_encrypt_auth_rounds_var(self._h, self._seal_key(pk48),
                                                                (ctypes.c_uint64 * max(n, 1))(*rounds),
                                                                _lib.buf(b"".join(sd)), _lib.buf(mb), cl, n, int(kdf), us, vs,
                                                                ws, ok))
        return self._encrypt_auth_var_result(n, lens, us, vs, ws, ok)

    def tlock_decrypt_auth_var(self, sig, us, vs, ws, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_auth_var: tlock_decrypt_auth over ciphertexts whose W values have ANY lengths (1 .. 256
        bytes each) in one call; msgs[i] has len(ws[i]) bytes where the item is good, else None."""
        sig = bytes(sig)
        if len(sig) != 96:
            raise ValueError("the round signature is 96 bytes")
        us = self._rows(us, 48, "U values")
        vs = self._rows(vs, _lib.V_LEN, "V values")
        n = len(us)
        wb, lens, cl = self._ragged(ws, "ciphertexts")
        if len(lens) != n or len(vs) != n:
            raise ValueError("one V and one W per U value")
        out, ok, cls = _lib.out_buf(len(wb)), _lib.out_buf(n), _lib.out_buf(n)
        sc = ctypes.c_uint8()
        rc = self.lib.blsv_tlock_decrypt_auth_var(self._h, _lib.buf(sig), _lib.buf(b"".join(us)), _lib.buf(b"".join(vs)),
                                                  _lib.buf(wb), cl, n, int(kdf), out, ok, cls,
                                                  ctypes.cast(ctypes.byref(sc), u8p))
        if rc == _lib.BLSV_EINVAL and sc.value:
            raise SignatureRejected(rc, self.lib.blsv_last_error(self._h).decode(), sc.value)
        self._check(rc)
        oks = [bool(x) for x in list(ok)[:n]]
        return TdecryptAuthResult(oks, list(cls)[:n], self._cut(out, lens, oks))

    def tlock_decrypt_auth_rounds_var(self, sigs, us_per_round, vs_per_round, ws_per_round, kdf=_lib.KDF_SHA256_CTR):
        """blsv_tlock_decrypt_auth_rounds_var: tlock_decrypt_auth_rounds with W values of any lengths, also inside
        one round's run. Returns TdecryptAuthRoundsResult in packed order."""
        runs = [self._rows(run, 48, "U values") for run in us_per_round]
        vruns = [self._rows(run, _lib.V_LEN, "V values") for run in vs_per_round]
        wruns = [list(run) for run in ws_per_round]
        if [len(r) for r in vruns] != [len(r) for r in runs] or [len(r) for r in wruns] != [len(r) for r in runs]:
            raise ValueError("one V and one W per U value, round by round")
        us = [u for run in runs for u in run]
        sb, counts, m = self._rounds_args(sigs, [len(run) for run in runs])
        n = len(us)
        wb, lens, cl = self._ragged([w for run in wruns for w in run], "ciphertexts")
        out, ok, cls, sc = _lib.out_buf(len(wb)), _lib.out_buf(n), _lib.out_buf(n), _lib.out_buf(m)
        self._check(self.lib.blsv_tlock_decrypt_auth_rounds_var(self._h, sb, counts, m, _lib.buf(b"".join(us)),
                                                                _lib.buf(b"".join(v for run in vruns for v in run)),
                                                                _lib.buf(wb), cl, n, int(kdf), out, ok, cls, sc))
        oks = [bool(x) for x in list(ok)[:n]]
        return TdecryptAuthRoundsResult(oks, list(cls)[:n], self._cut(out, lens, oks), list(sc)[:m])

    # ------------------------------------------------------------------ stage profiling
    STAGES = ("hash", "decompress", "miller", "final_exp", "finish", "lat", "rlc", "tlock")

    def profile(self, on=True):
        self._check(self.lib.blsv_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        """{stage: (summed ms, launches, items)} since the last read (HIP events on the launch stream)."""
        n = len(self.STAGES)
        ms = (ctypes.c_double * n)()
        la = (ctypes.c_uint64 * n)()
        it = (ctypes.c_uint64 * n)()
        rc = self.lib.blsv_profile_read(self._h, ms, la, it, n)
        if rc < 0:
            raise EngineError(rc, self.lib.blsv_last_error(self._h).decode())
        return {s: (ms[k], la[k], it[k]) for k, s in enumerate(self.STAGES)}

    LAT_MARKS = ("start", "hash", "sig_decoded", "sig_miller", "phase_a", "key_miller", "miller_product",
                 "final_exp", "pow1_start", "pow1_end", "xmd_done", "sswu_done", "iso_add_done", "cofactor_done",
                 "sig_sqrt_done", "sig_subgroup_done")

    def lat_trace_enable(self, on=True):
        """Turn the latency kernel's phase marks on or off (a device-global flag, off by default)."""
        self._check(self.lib.blsv_lat_trace_enable(self._h, 1 if on else 0))

    def lat_trace(self, clear=True):
        """Phase marks (microseconds from the first mark) of item 0 of the last latency-path launch
        while marks are enabled (blsv_lat_trace_enable, blsv_lat_trace); marks never stamped are left
        out."""
        n = len(self.LAT_MARKS)
        t = (ctypes.c_uint64 * n)()
        rate = ctypes.c_double()
        got = self.lib.blsv_lat_trace(self._h, t, n, ctypes.byref(rate), 1 if clear else 0)
        if got < 0:
            raise EngineError(got, self.lib.blsv_last_error(self._h).decode())
        t0 = t[0]
        return {k: (t[i] - t0) / rate.value for i, k in enumerate(self.LAT_MARKS[:got]) if t[i] and t0}

    # ------------------------------------------------------------------ testing hooks
    def set_lat_max(self, n):
        """Batches of at most n items take the latency path (one 8-wave workgroup per item; default
        1,536, clamped to the chunk); returns the old cutover."""
        return self.lib.blsv_set_lat_max(self._h, int(n))

    def set_chunk(self, items):
        """Cap the items per pipeline pass (~42.4 KB of HBM staging per item; 0 = the default 2^20);
        returns the previous chunk (blsv_set_chunk)."""
        return self.lib.blsv_set_chunk(self._h, int(items))

    def workspace_bytes(self):
        """HBM bytes of pipeline staging this context holds (blsv_workspace_bytes)."""
        return self.lib.blsv_workspace_bytes(self._h)

    def test_fp_mul(self, a_limbs, b_limbs):
        n = len(a_limbs) // 12
        A = (ctypes.c_uint32 * max(len(a_limbs), 1))(*a_limbs)
        B = (ctypes.c_uint32 * max(len(b_limbs), 1))(*b_limbs)
        O = (ctypes.c_uint32 * max(n * 12, 1))()
        self._check(self.lib.blsv_test_fp_mul(self._h, A, B, n, O))
        return list(O)[:n * 12]

    def test_ops(self):
        """{name: (Fp elements in, Fp elements out, lanes per item)} of blsv_test_op."""
        ops, k = {}, 0
        name, a, b, c = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        while self.lib.blsv_test_op_info(k, ctypes.byref(name), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0:
            ops[name.value.decode()] = (a.value, b.value, c.value)
            k += 1
        return ops

    def test_op(self, name, operands):
        """blsv_test_op: one raw device operation on len(operands) / in_fp items. operands: a flat list
        of Fp elements as Python integers below 2^384, each standing for its 12 raw words (tower order
        within an item, items one after the other); returns the raw result elements the same way.
        Nothing is converted or reduced on the way in or out."""
        if self._ops is None:
            self._ops = self.test_ops()
        nin, nout, _ = self._ops[name]
        if len(operands) % nin:
            raise ValueError(f"{name} takes {nin} Fp elements per item")
        n = len(operands) // nin
        raw = b"".join(int(v).to_bytes(48, "little") for v in operands)
        A = (ctypes.c_uint32 * max(len(raw) // 4, 1)).from_buffer_copy(raw if raw else bytes(4))
        O = (ctypes.c_uint32 * max(n * nout * 12, 1))()
        self._check(self.lib.blsv_test_op(self._h, name.encode(), A, n, O))
        ob = bytes(O)
        return [int.from_bytes(ob[48 * k:48 * k + 48], "little") for k in range(n * nout)]

    def test_pairing(self, p_words, q_words):
        n = len(p_words) // 24
        Pp = (ctypes.c_uint32 * max(len(p_words), 1))(*p_words)
        Q = (ctypes.c_uint32 * max(len(q_words), 1))(*q_words)
        O = (ctypes.c_uint32 * max(n * 144, 1))()
        self._check(self.lib.blsv_test_pairing(self._h, Pp, Q, n, O))
        return list(O)[:n * 144]

    def test_final_exp(self, f_words):
        """(production stage, one-lane reference) final exponentiations of n Fp12 (144 raw words each)."""
        n = len(f_words) // 144
        Fw = (ctypes.c_uint32 * max(len(f_words), 1))(*f_words)
        A = (ctypes.c_uint32 * max(n * 144, 1))()
        B = (ctypes.c_uint32 * max(n * 144, 1))()
        self._check(self.lib.blsv_test_final_exp(self._h, Fw, n, A, B))
        return list(A)[:n * 144], list(B)[:n * 144]

    def test_tail_split(self, q):
        """The round a pass is split by (blsv_test_tail_split): q items, 0 = never split, None = the
        device's own round (one single-lane f-pass wave on every SIMD)."""
        self._check(self.lib.blsv_test_tail_split(self._h, ctypes.c_size_t(-1).value if q is None else int(q)))

    def test_hash_to_g2(self, msgs):
        n = len(msgs)
        lens = (ctypes.c_uint32 * max(n, 1))(*[len(m) for m in msgs])
        O = (ctypes.c_uint32 * max(n * 48, 1))()
        inf = _lib.out_buf(n)
        self._check(self.lib.blsv_test_hash_to_g2(self._h, _lib.buf(b"".join(bytes(m) for m in msgs)), lens, n, O,
                                                  inf))
        return list(O)[:n * 48], list(inf)[:n]

    def spec_stats(self):
        """(kept, recomputed) speculative recoveries of this context (blsv_test_spec_stats)."""
        h, m = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.blsv_test_spec_stats(self._h, ctypes.byref(h), ctypes.byref(m)))
        return h.value, m.value

    def test_generic_chains(self, on=True):
        """Every hash's cofactor clearing and every signature's subgroup check through the generic
        formulas (k_hash_cofactor_generic, k_subgroup_g2_generic) instead of only the lanes the
        call-free chains flag; process-global, for the parity tests."""
        self._check(self.lib.blsv_test_generic_chains(self._h, 1 if on else 0))


def verify_chained_multi(engines, first_round, prev0, sigs, counts=None):
    """blsv_verify_chained_multi: the chained range split into contiguous shards over several
    Engines (one per GPU; each holds the same group), verified concurrently (one host thread per
    context inside the library) and merged: the BatchResult of one verify_chained over the whole
    range. counts: shard lengths (None = even split)."""
    if not engines:
        raise ValueError("verify_chained_multi needs at least one engine")
    lib = engines[0].lib
    n = len(sigs)
    if any(len(s) != 96 for s in sigs):
        raise ValueError("chained signatures must be 96 bytes (reject wrong lengths host-side)")
    sigb = b"".join(bytes(s) for s in sigs)
    hs = (ctypes.c_void_p * len(engines))(*[e._h.value for e in engines])
    cs = None if counts is None else (ctypes.c_size_t * len(engines))(*counts)
    bm = _lib.out_buf((n + 7) // 8)
    fb = ctypes.c_uint64()
    cls = _lib.out_buf(n)
    rc = lib.blsv_verify_chained_multi(hs, len(engines), cs, first_round, _lib.buf(prev0), len(prev0), _lib.buf(sigb),
                                       n, bm, ctypes.byref(fb), cls)
    if rc != 0:
        msgs = "; ".join(lib.blsv_last_error(e._h).decode(errors="replace") for e in engines)
        raise EngineError(rc, f"blsv_verify_chained_multi failed: {msgs}")
    return BatchResult(_bits(bm, n), None if fb.value == 2 ** 64 - 1 else fb.value, list(cls)[:n])


class Service:
    """Thread-safe front end (blsv_service_*): any number of threads call verify_partial /
    verify_recovered at once; items that arrive together are verified in one launch. ctypes releases
    the GIL for the duration of each call, so Python threads block in C side by side."""

    def __init__(self, device: int = 0, gap_us: int = 0, max_wait_us: int = 0, init_torch: bool = True):
        if init_torch:
            try:
                import torch
            except ImportError:
                torch = None
            if torch is not None:
                torch.cuda.set_device(int(device))
                torch.zeros(1, device=torch.device("cuda", int(device)))
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.blsv_service_create(int(device), int(gap_us), int(max_wait_us), ctypes.byref(h))
        if rc != 0:
            raise EngineError(rc, f"blsv_service_create(device={device}) failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.blsv_service_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def verify_partial(self, commits, n, msg, partial):
        """key.Scheme.VerifyPartial(pubPoly, msg, partial): (ok, reject class)."""
        cb = b"".join(bytes(c) for c in commits)
        ok, cls = ctypes.c_uint8(), ctypes.c_uint8()
        p = bytes(partial)
        rc = self.lib.blsv_service_verify_partial(self._h, _lib.buf(cb), len(commits), int(n), _lib.buf(msg), len(msg),
                                                  _lib.buf(p), len(p), ctypes.byref(ok), ctypes.byref(cls))
        if rc != 0:
            raise EngineError(rc, "blsv_service_verify_partial failed")
        return bool(ok.value), cls.value

    def prepare_partial(self, commits, n, msg, partial):
        """A zero-argument callable doing exactly the ctypes call of verify_partial, its arguments
        marshalled in advance (so concurrent Python callers hold the GIL only for the call itself)."""
        cb = _lib.buf(b"".join(bytes(c) for c in commits))
        mb, pb = _lib.buf(msg), _lib.buf(bytes(partial))
        t, ml, pl = len(commits), len(msg), len(partial)
        ok, cls = ctypes.c_uint8(), ctypes.c_uint8()
        f, h, pok, pcls = self.lib.blsv_service_verify_partial, self._h, ctypes.byref(ok), ctypes.byref(cls)

        def call():
            rc = f(h, cb, t, n, mb, ml, pb, pl, pok, pcls)
            if rc != 0:
                raise EngineError(rc, "blsv_service_verify_partial failed")
            return bool(ok.value), cls.value

        return call

    def verify_recovered(self, pk48, msg, sig96):
        """key.Scheme.VerifyRecovered(pub, msg, sig): (ok, reject class)."""
        ok, cls = ctypes.c_uint8(), ctypes.c_uint8()
        rc = self.lib.blsv_service_verify_recovered(self._h, _lib.buf(pk48), _lib.buf(msg), len(msg), _lib.buf(sig96),
                                                    ctypes.byref(ok), ctypes.byref(cls))
        if rc != 0:
            raise EngineError(rc, "blsv_service_verify_recovered failed")
        return bool(ok.value), cls.value

    def test_limits(self, chunk=0, lat_max=(1 << 64) - 1, arena_entries=0):
        """blsv_test_service_limits: shrink the dispatcher's pass size / cutover / key arena (tests of
        the multi-pass and arena-overflow paths); returns the device batches run so far."""
        n = ctypes.c_uint64()
        rc = self.lib.blsv_test_service_limits(self._h, int(chunk), int(lat_max), int(arena_entries), ctypes.byref(n))
        if rc != 0:
            raise EngineError(rc, "blsv_test_service_limits failed")
        return n.value

    def stats(self):
        """(launches, items, largest batch) since creation."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.lib.blsv_service_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value


def limbs_of(v, n=12):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def int_of(limbs):
    return sum(int(x) << (32 * i) for i, x in enumerate(limbs))
