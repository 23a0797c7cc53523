#!/usr/bin/env python3
"""The authenticated timelock on the latency path against the batch path on one MI355X (not part of bench.py:
no headline number comes from here). Everything is measured in ONE run through the HOST forms
(blsv_tlock_decrypt_auth, _rounds, blsv_tlock_encrypt_auth, _rounds) of one context, with a host clock around
the call (a host form returns when its outputs are written); the two modes -- blsv_set_tauth_lat_max 0 (off: the
batch path, the parent's code) and on -- alternate call by call; after warm-up pairs, medians. In every
comparison the two modes must return identical bytes, ok and classes, or the run is void (exit status 1).

Inputs at mlen = 32: 64 rounds signed with the golden chain's key (MessageV2, as a beacon signs them), 4096
ciphertexts made by the batch path's own blsv_tlock_encrypt_auth (round j's 64 under round j; all 4096 under
round 1 as well), seeded seeds and messages.

  a  a lone decrypt_auth, a new sigma every call (mode off's one-entry sigma cache never hits)
  b  a lone decrypt_auth, the same sigma every call
  c  a lone encrypt_auth to a new round every call, and to the same round every call
  d  64 items of 64 rounds through each rounds form
  e  the sweep n = 1 .. 4096 of both directions (one round); the crossover is the smallest n at which mode off
     is faster: what blsv_set_tauth_lat_max should be given
  f  in the same run the lone unauthenticated blsv_tlock_decrypt / blsv_tlock_encrypt on THEIR latency paths:
     the difference to (b) / (c, same round) is what authentication costs on this path
  w  (a), (b) with the check's walk on one wave instead of eight (blsv_test_tauth_walk_waves), alternating
     call by call with the eight-wave form

PREDICTION, written before the first run (nothing below had been measured by anyone):
  decrypt  the unauthenticated lone decrypt's 1.53 ms plus the tail. The tail is about thirty
           SHA-256 compressions and one 256-step reduction as single-lane-rate work, ~3 us each: ~0.1 ms; the walk
           at an eighth of 8.6's 511 us for 64 non-zero digits, ~65 us, plus three complete additions at ~15
           products each, ~10 us, plus team syncs: ~0.08 ms; the comparison and stores ~0.02 ms. So (b) ~1.75 ms,
           (a) the same (the path has no sigma cache), against 14 - 18 ms in mode off: 8 - 10 times. The one-wave
           walk should cost ~0.45 ms more than the eight-wave one: (w) ~2.2 ms.
  encrypt  the unauthenticated lone encrypt's 1.89 ms plus the derivation in front of the hash on every wave
           (~6 compressions and the reduction, ~0.03 ms) plus the midstate, H2 and H4 on one lane behind the final
           exponentiation (~12 compressions, ~0.05 ms), minus the 576-byte encoding: ~1.95 ms new or same round,
           against ~35 ms (new round) and ~5.3 ms (same round) in mode off.
  d        ~1.8 / ~2.0 ms against ~17 / ~18 ms.
  e        crossovers where the unauthenticated paths have theirs: 2048 - 4096 (decrypt), 512 - 1024 (encrypt).

    python tools/tauth_lat_bench.py            # writes profiles/tauth_lat_bench.json on an MI355X
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NSIG, NMAX, MLEN = 64, 4096, 32
PREDICTION_MS = {"a_on": 1.75, "b_on": 1.75, "c_new_round_on": 1.95, "c_same_round_on": 1.95, "d_decrypt_on": 1.8,
                 "d_encrypt_on": 2.0, "f_auth_cost_decrypt": 0.22, "f_auth_cost_encrypt": 0.06,
                 "w_one_wave_minus_eight": 0.45}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=48, help="pairs of calls per lone measurement")
    ap.add_argument("--sweep-reps", type=int, default=5, help="pairs of calls per n of a sweep")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib
    from drand_amd.engine import Engine
    from oracle import bls12381 as O

    if not torch.cuda.is_available():
        raise SystemExit("tauth_lat_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    lib, h = eng.lib, eng.handle
    KDF = _lib.KDF_SHA256_CTR

    rng = np.random.default_rng(5)
    seeds = np.ascontiguousarray(rng.integers(0, 256, NMAX * 32, dtype=np.uint8))
    msgs = np.ascontiguousarray(rng.integers(0, 256, NMAX * MLEN, dtype=np.uint8))
    rounds = np.ascontiguousarray(np.repeat(np.arange(1, NSIG + 1, dtype=np.uint64), NMAX // NSIG))
    sk = int(ch["sk"], 16).to_bytes(32, "big")
    sig_list = eng.sign(sk, [O.message_v2(r) for r in range(1, NSIG + 1)])
    sigs = np.frombuffer(b"".join(bytes(s) for s in sig_list), dtype=np.uint8).copy()
    assert len(sigs) == 96 * NSIG

    def p8(a, off=0):
        return ctypes.cast(a.ctypes.data + off, _lib.u8p)

    class Ct:  # a ciphertext set, or an encrypting call's outputs
        def __init__(self, n):
            self.us = np.empty(48 * n, dtype=np.uint8)
            self.vs = np.empty(32 * n, dtype=np.uint8)
            self.ws = np.empty(MLEN * n, dtype=np.uint8)
            self.ok = np.empty(n, dtype=np.uint8)

        def arrays(self):
            return self.us, self.vs, self.ws, self.ok

        def good(self):
            return bool(self.ok.min() == 1)

    class Pt:  # a decrypting call's outputs
        def __init__(self, n, m=1):
            self.out = np.empty(MLEN * n, dtype=np.uint8)
            self.ok = np.empty(n, dtype=np.uint8)
            self.cls = np.empty(n, dtype=np.uint8)
            self.sc = np.empty(m, dtype=np.uint8)

        def arrays(self):
            return self.out, self.ok, self.cls, self.sc

        def good(self):
            return bool(self.ok.min() == 1 and self.sc.max() == 0)

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays()))

    def enc(rnd, at, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_encrypt_auth(h, None, int(rnd), p8(seeds, 32 * at), p8(msgs, MLEN * at), MLEN, n, KDF, p8(o.us),
                                         p8(o.vs), p8(o.ws), p8(o.ok))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_encrypt_auth failed: %d" % rc)
        return dt

    def enc_rounds(at, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_encrypt_auth_rounds(h, None, ctypes.cast(rounds.ctypes.data + 8 * at, _lib.u64p), p8(seeds, 32 * at),
                                                p8(msgs, MLEN * at), MLEN, n, KDF, p8(o.us), p8(o.vs), p8(o.ws), p8(o.ok))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_encrypt_auth_rounds failed: %d" % rc)
        return dt

    # the ciphertexts, by the batch path: per_round[i] under round rounds[i]; one_round[i] under round 1
    eng.set_tauth_lat_max(0, 0)
    per_round, one_round = Ct(NMAX), Ct(NMAX)
    enc_rounds(0, NMAX, per_round)
    enc(1, 0, NMAX, one_round)
    made = per_round.good() and one_round.good()

    def dec(ct, j, at, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_decrypt_auth(h, p8(sigs, 96 * j), p8(ct.us, 48 * at), p8(ct.vs, 32 * at), p8(ct.ws, MLEN * at), MLEN,
                                         n, KDF, p8(o.out), p8(o.ok), p8(o.cls), p8(o.sc))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_decrypt_auth failed: %d" % rc)
        return dt

    counts64 = np.ones(NSIG, dtype=np.uint64)
    d_idx = np.arange(NSIG) * (NMAX // NSIG)  # one item of every round
    d_ct = Ct(NSIG)
    for name in ("us", "vs", "ws"):
        w = {"us": 48, "vs": 32, "ws": MLEN}[name]
        getattr(d_ct, name)[:] = getattr(per_round, name).reshape(NMAX, w)[d_idx].reshape(-1)

    def dec_rounds(o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_decrypt_auth_rounds(h, p8(sigs), counts64.ctypes.data_as(_lib.u64p), NSIG, p8(d_ct.us), p8(d_ct.vs),
                                                p8(d_ct.ws), MLEN, NSIG, KDF, p8(o.out), p8(o.ok), p8(o.cls), p8(o.sc))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_decrypt_auth_rounds failed: %d" % rc)
        return dt

    state = {"same": True, "good": True}

    def pairs(call, make, reps, warmup, off=lambda: eng.set_tauth_lat_max(0, 0), on=lambda: eng.set_tauth_lat_max(NMAX, NMAX)):
        """reps pairs (mode off, mode on) of call(k, out) after warmup pairs; every pair compared"""
        a, b = make(), make()
        t_offs, t_ons = [], []
        for k in range(warmup + reps):
            off()
            t_off = call(k, a)
            on()
            t_on = call(k, b)
            state["same"] &= same(a, b)
            state["good"] &= a.good()
            if k >= warmup:
                t_offs.append(t_off)
                t_ons.append(t_on)
        eng.set_tauth_lat_max(0, 0)
        mo, mn = statistics.median(t_offs), statistics.median(t_ons)
        return {"off_ms_median": round(mo, 4), "on_ms_median": round(mn, 4), "off_over_on": round(mo / mn, 2),
                "off_ms_min": round(min(t_offs), 4), "on_ms_min": round(min(t_ons), 4), "pairs": reps}

    def sweep(call, make, tag):
        rows, cross = [], None
        n = 1
        while n <= NMAX:
            r = pairs(lambda k, o, n=n: call(n, o), lambda n=n: make(n), args.sweep_reps, 2)
            r["n"] = n
            rows.append(r)
            if cross is None and r["off_ms_median"] < r["on_ms_median"]:
                cross = n
            print(tag, r, file=sys.stderr, flush=True)
            n *= 2
        return rows, cross

    def show(tag, r):
        print(tag, r, file=sys.stderr, flush=True)
        return r

    t0s = (eng.tauth_lat_stats(), eng.tlock_stats(), eng.tlock_seal_stats(), eng.tlock_lat_stats(), eng.tseal_lat_stats())
    per = NMAX // NSIG
    res_a = show("a", pairs(lambda k, o: dec(per_round, k % NSIG, (k % NSIG) * per + (k // NSIG) % per, 1, o), lambda: Pt(1),
                            args.reps, args.warmup))
    res_b = show("b", pairs(lambda k, o: dec(one_round, 0, k % NMAX, 1, o), lambda: Pt(1), args.reps, args.warmup))
    res_c_new = show("c new", pairs(lambda k, o: enc((1 << 32) + k, k % NMAX, 1, o), lambda: Ct(1), args.reps, args.warmup))
    res_c_same = show("c same", pairs(lambda k, o: enc(7, k % NMAX, 1, o), lambda: Ct(1), args.reps, args.warmup))
    res_d_dec = show("d dec", pairs(lambda k, o: dec_rounds(o), lambda: Pt(NSIG, NSIG), max(args.sweep_reps, 9), 2))
    # 64 items of 64 rounds: the seeds and messages d_idx picks, packed
    s64 = np.ascontiguousarray(seeds.reshape(NMAX, 32)[d_idx].reshape(-1))
    m64 = np.ascontiguousarray(msgs.reshape(NMAX, MLEN)[d_idx].reshape(-1))
    r64 = np.ascontiguousarray(rounds[d_idx])

    def enc_rounds_64(o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_encrypt_auth_rounds(h, None, r64.ctypes.data_as(_lib.u64p), p8(s64), p8(m64), MLEN, NSIG, KDF,
                                                p8(o.us), p8(o.vs), p8(o.ws), p8(o.ok))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_encrypt_auth_rounds failed: %d" % rc)
        return dt
    res_d_enc = show("d enc", pairs(lambda k, o: enc_rounds_64(o), lambda: Ct(NSIG), max(args.sweep_reps, 9), 2))
    sweep_dec, cross_dec = sweep(lambda n, o: dec(one_round, 0, 0, n, o), lambda n: Pt(n), "e dec")
    sweep_enc, cross_enc = sweep(lambda n, o: enc(7, 0, n, o), lambda n: Ct(n), "e enc")
    t1s = (eng.tauth_lat_stats(), eng.tlock_stats(), eng.tlock_seal_stats(), eng.tlock_lat_stats(), eng.tseal_lat_stats())

    # f: the unauthenticated lone calls on their own latency paths, in the same run
    class Plain:
        def __init__(self):
            self.us = np.empty(48, dtype=np.uint8)
            self.out = np.empty(MLEN, dtype=np.uint8)
            self.ok = np.empty(1, dtype=np.uint8)
            self.cls = np.empty(1, dtype=np.uint8)
            self.sc = np.empty(1, dtype=np.uint8)

    def median_of(call, reps, warmup):
        ts = [call(k) for k in range(warmup + reps)][warmup:]
        return round(statistics.median(ts), 4)
    pl = Plain()

    def plain_enc(k):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_encrypt(h, None, 7, p8(seeds, 32 * (k % NMAX)), p8(msgs, MLEN * (k % NMAX)), MLEN, 1, KDF, p8(pl.us),
                                    p8(pl.out), p8(pl.ok))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_encrypt failed: %d" % rc)
        return dt

    def plain_dec(k):
        at = k % NMAX
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_decrypt(h, p8(sigs), p8(one_round.us, 48 * at), p8(one_round.ws, MLEN * at), MLEN, 1, KDF, p8(pl.out),
                                    p8(pl.ok), p8(pl.cls), p8(pl.sc))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_decrypt failed: %d" % rc)
        return dt
    eng.set_tlock_lat_max(NMAX)
    eng.set_tseal_lat_max(NMAX)
    f_dec = median_of(plain_dec, args.reps, args.warmup)
    f_enc = median_of(plain_enc, args.reps, args.warmup)
    eng.set_tlock_lat_max(0)
    eng.set_tseal_lat_max(0)
    res_f = {"plain_decrypt_lat_ms_median": f_dec, "plain_encrypt_lat_ms_median": f_enc,
             "auth_cost_decrypt_ms": round(res_b["on_ms_median"] - f_dec, 4),
             "auth_cost_encrypt_ms": round(res_c_same["on_ms_median"] - f_enc, 4)}
    print("f", res_f, file=sys.stderr, flush=True)

    # w: both modes on the latency path; "off" = the one-wave walk, "on" = the eight-wave walk
    def walk(w):
        eng.set_tauth_lat_max(NMAX, NMAX)
        eng.test_tauth_walk_waves(w)
    res_w_a = show("w a", pairs(lambda k, o: dec(per_round, k % NSIG, (k % NSIG) * per + (k // NSIG) % per, 1, o), lambda: Pt(1),
                                args.reps, args.warmup, off=lambda: walk(1), on=lambda: walk(8)))
    res_w_b = show("w b", pairs(lambda k, o: dec(one_round, 0, k % NMAX, 1, o), lambda: Pt(1), args.reps, args.warmup,
                                off=lambda: walk(1), on=lambda: walk(8)))
    eng.test_tauth_walk_waves(8)
    eight_faster = all(r["on_ms_median"] < r["off_ms_median"] * 0.98 for r in (res_w_a, res_w_b))

    half = all(r["on_ms_median"] * 2 <= r["off_ms_median"] for r in (res_a, res_b, res_d_dec, res_d_enc, res_c_new))
    below = res_c_same["on_ms_median"] < res_c_same["off_ms_median"] * 0.98

    def recommend(cross):
        return (cross // 2 if cross else NMAX) if half and below else None
    res = {"tool": "tools/tauth_lat_bench.py", "device": torch.cuda.get_device_name(0), "mlen": MLEN, "warmup": args.warmup,
           "timing": "host clock around the host-form call (it returns with its outputs written); mode off = "
                     "blsv_set_tauth_lat_max(0, 0), the batch path; mode on = blsv_set_tauth_lat_max(4096, 4096); the modes "
                     "alternate call by call; medians",
           "prediction_ms_written_before_the_run": PREDICTION_MS,
           "a_lone_decrypt_new_sigma_every_call": res_a, "b_lone_decrypt_same_sigma": res_b,
           "c_lone_encrypt_new_round_every_call": res_c_new, "c_lone_encrypt_same_round": res_c_same,
           "d_64_items_of_64_rounds_decrypt": res_d_dec, "d_64_items_of_64_rounds_encrypt": res_d_enc,
           "e_decrypt_sweep": sweep_dec, "e_crossover_n_decrypt": cross_dec, "e_encrypt_sweep": sweep_enc,
           "e_crossover_n_encrypt": cross_enc, "f_unauthenticated_on_their_latency_paths": res_f,
           "w_walk_one_wave_as_off_eight_waves_as_on": {"a": res_w_a, "b": res_w_b,
                                                       "eight_faster_by_more_than_2_percent": eight_faster},
           "acceptance_on_at_most_half_of_off_in_a_b_d_and_c_new_round": half,
           "acceptance_on_below_off_by_more_than_2_percent_in_c_same_round": below,
           "recommended_tauth_lat_max_open_seal": [recommend(cross_dec), recommend(cross_enc)],
           "same_bytes_ok_and_classes_in_every_pair": state["same"], "all_good": state["good"] and made,
           "tauth_lat_stats_moved_by": [y - x for x, y in zip(t0s[0], t1s[0])],
           "tlock_stats_moved_by": [y - x for x, y in zip(t0s[1], t1s[1])],
           "tlock_seal_stats_moved_by": [y - x for x, y in zip(t0s[2], t1s[2])],
           "tlock_lat_stats_moved_by": [y - x for x, y in zip(t0s[3], t1s[3])],
           "tseal_lat_stats_moved_by": [y - x for x, y in zip(t0s[4], t1s[4])]}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    path = args.out or (os.path.join(ROOT, "profiles", "tauth_lat_bench.json") if on_mi355x else None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if state["same"] and state["good"] and made else 1


if __name__ == "__main__":
    sys.exit(main())
