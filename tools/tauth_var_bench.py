#!/usr/bin/env python3
"""The authenticated timelock with mixed message lengths in one call (blsv_tlock_*_auth_var) on one MI355X (not
part of bench.py: no headline number comes from here). One context, the HOST forms, a host clock around each
side (a host form returns when its outputs are written). The two sides of a comparison alternate call by call;
after a warm-up pair, five pairs; medians. The outputs of the two sides are compared byte for byte and hashed.

  a  what the feature buys: 65,536 items with lengths uniform in 1 .. 256 (seeded), ONE _var call against the 256
     per-length calls callers.timelock_*_auth make today (the engine calls alone: the per-length inputs are
     gathered before the clock starts, so callers' Python list partitioning comes on top of the per-length side).
     Decrypt and encrypt; the latency switch off, and on at the recommended (1024, 512), where the ~256-item
     per-length calls route to the latency path and the one _var call stays on the batch path.
  b  what raggedness costs: (b1) the same 65,536 items at a uniform 32 bytes through the _var entry against the
     uniform entry -- the same kernels' work, the offset table and its upload added; (b2) the mixed-length call
     against a uniform call of the same item count and (within half a percent) the same total bytes, mlen = 129,
     the byte form on both sides -- what the lanes of a wave running 1 .. 8 pieces each cost.

PREDICTION, written before the first run (nobody had measured this path):
  b  the tails are ~4% of a decrypt pass (+4.05%), and of that the walk of 653 Fp products is
     length-independent; the SHA work that does depend on the length is a few percent of the tail. A wave of the
     ragged kernels leaves its piece loops with its longest item, 8 pieces almost always, against 4 - 5 on
     average: at worst the hashing part of the tail doubles, well below 1% of a pass. The offset table is 4 bytes
     per item beside ~300 bytes per item of traffic. So b1 and b2 should both sit inside the ~3% box-to-box spread
     of DESIGN.md 4.4: ratios 0.97 .. 1.03.
  a  the per-length side pays the call floor 256 times: 14 - 19 ms under a cached signature decrypting (8.9), ~5 ms
     to a cached round encrypting, each plus ~256 items of work -- ~4 - 5 s and ~1.5 s; the one call is 65,536
     items of a ~300 ms-per-Mi pass plus one floor: ~35 ms decrypting, ~25 ms encrypting. So ~100 times and ~60
     times with the switch off. With the switch on a 256-item call costs a few waves of workgroups, ~3 - 6 ms:
     256 of them ~1 s, still ~30 times the one call.

    python tools/tauth_var_bench.py            # writes profiles/tauth_var_bench.json on an MI355X
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, ROUND, UNIFORM, SAME_BYTES_MLEN = 65536, 7, 32, 129
LAT_ON = (1024, 512)
PREDICTION = {"b1_var_over_uniform": [0.97, 1.03], "b2_mixed_over_uniform_same_bytes": [0.97, 1.03],
              "a_decrypt_per_length_over_var_switch_off": 100, "a_encrypt_per_length_over_var_switch_off": 60,
              "a_per_length_over_var_switch_on": 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib
    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tauth_var_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    sig = [bytes.fromhex(b["sig_v2"]) for b in ch["beacons"] if b.get("sig_v2") and b["round"] == ROUND][0]
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    lib, h = eng.lib, eng.handle
    KDF = _lib.KDF_SHA256_CTR
    sigb = _lib.buf(sig)

    def p8(a, off=0):
        return ctypes.cast(a.ctypes.data + off, _lib.u8p)

    def p32(a):
        return ctypes.cast(a.ctypes.data, _lib.u32p)

    rng = np.random.default_rng(11)
    seeds = np.ascontiguousarray(rng.integers(0, 256, N * 32, dtype=np.uint8))

    class Set:
        """n items of the lengths `lens` packed back to back: messages, and room for the ciphertexts and verdicts."""

        def __init__(self, lens, seed_rows=None):
            self.lens = np.ascontiguousarray(lens, dtype=np.uint32)
            self.n = len(self.lens)
            self.total = int(self.lens.sum(dtype=np.uint64))
            self.seeds = seeds if seed_rows is None else np.ascontiguousarray(seeds.reshape(N, 32)[seed_rows].reshape(-1))
            self.msgs = np.ascontiguousarray(rng.integers(0, 256, self.total, dtype=np.uint8))
            self.us, self.vs = np.zeros(48 * self.n, dtype=np.uint8), np.zeros(32 * self.n, dtype=np.uint8)
            self.ws, self.ok = np.zeros(self.total, dtype=np.uint8), np.zeros(self.n, dtype=np.uint8)
            self.out, self.dok = np.zeros(self.total, dtype=np.uint8), np.zeros(self.n, dtype=np.uint8)
            self.cls, self.sc = np.zeros(self.n, dtype=np.uint8), np.zeros(1, dtype=np.uint8)

        def uniform(self):
            assert int(self.lens.min()) == int(self.lens.max())
            return int(self.lens[0])

        def enc_var(self):
            return lib.blsv_tlock_encrypt_auth_var(h, None, ROUND, p8(self.seeds), p8(self.msgs), p32(self.lens), self.n, KDF,
                                                   p8(self.us), p8(self.vs), p8(self.ws), p8(self.ok))

        def enc_uniform(self):
            return lib.blsv_tlock_encrypt_auth(h, None, ROUND, p8(self.seeds), p8(self.msgs), self.uniform(), self.n, KDF,
                                               p8(self.us), p8(self.vs), p8(self.ws), p8(self.ok))

        def dec_var(self):
            return lib.blsv_tlock_decrypt_auth_var(h, sigb, p8(self.us), p8(self.vs), p8(self.ws), p32(self.lens), self.n, KDF,
                                                   p8(self.out), p8(self.dok), p8(self.cls), p8(self.sc))

        def dec_uniform(self):
            return lib.blsv_tlock_decrypt_auth(h, sigb, p8(self.us), p8(self.vs), p8(self.ws), self.uniform(), self.n, KDF,
                                               p8(self.out), p8(self.dok), p8(self.cls), p8(self.sc))

        def enc_outputs(self):
            return self.us, self.vs, self.ws, self.ok

        def dec_outputs(self):
            return self.out, self.dok, self.cls

        def take_ciphertexts(self, other, rows=None, byte_idx=None):
            """the ciphertexts `other` made, whole or the rows / bytes given"""
            self.us[:] = other.us if rows is None else other.us.reshape(-1, 48)[rows].reshape(-1)
            self.vs[:] = other.vs if rows is None else other.vs.reshape(-1, 32)[rows].reshape(-1)
            self.ws[:] = other.ws if byte_idx is None else other.ws[byte_idx]

    def check(rc, what):
        if rc:
            raise SystemExit("%s failed: %d (%s)" % (what, rc, lib.blsv_last_error(h).decode()))

    def timed(calls):
        t0 = time.perf_counter()
        for what, c in calls:
            check(c(), what)
        return (time.perf_counter() - t0) * 1e3

    state = {"same": True, "good": True}

    def digest(arrays):
        d = hashlib.sha256()
        for a in arrays:
            d.update(a.tobytes())
        return d.hexdigest()

    def compare(side_a, side_b, outputs_a, outputs_b, good, tag):
        """args.pairs pairs (a, b) after the warm-up; outputs_x() -> the arrays to compare after each pair"""
        ta, tb, ha, hb = [], [], None, None
        for k in range(args.warmup + args.pairs):
            t_a = timed(side_a)
            t_b = timed(side_b)
            oa, ob = outputs_a(), outputs_b()
            if oa is not None:
                state["same"] &= all(np.array_equal(x, y) for x, y in zip(oa, ob))
                ha, hb = digest(oa), digest(ob)
            state["good"] &= good()
            if k >= args.warmup:
                ta.append(t_a)
                tb.append(t_b)
        ma, mb = statistics.median(ta), statistics.median(tb)
        r = {"a_ms_median": round(ma, 3), "b_ms_median": round(mb, 3), "a_over_b": round(ma / mb, 4),
             "a_ms_all": [round(t, 3) for t in ta], "b_ms_all": [round(t, 3) for t in tb], "pairs": args.pairs,
             "sha256_a": ha, "sha256_b": hb}
        print(tag, r, file=sys.stderr, flush=True)
        return r

    # ---- the inputs
    lens = rng.integers(1, 257, N, dtype=np.uint32)
    mixed = Set(lens)
    offs = np.zeros(N + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens, dtype=np.int64)
    groups = []  # per distinct length: a Set of its items, their rows and their byte indices in the packed order
    for mlen in range(1, 257):
        rows = np.nonzero(lens == mlen)[0]
        if not len(rows):
            continue
        byte_idx = (offs[rows][:, None] + np.arange(mlen)[None, :]).reshape(-1)
        g = Set(np.full(len(rows), mlen, dtype=np.uint32), seed_rows=rows)
        g.msgs[:] = mixed.msgs[byte_idx]
        groups.append((g, rows, byte_idx))
    eng.set_tauth_lat_max(0, 0)
    check(mixed.enc_var(), "encrypt_auth_var")  # the ciphertexts both decrypting sides open
    for g, rows, byte_idx in groups:
        g.take_ciphertexts(mixed, rows, byte_idx)

    def gathered(arrays_of, kinds):
        """the per-length sides' outputs in the one call's packed order"""
        outs = []
        for kind, name in kinds:
            full = np.zeros_like(getattr(mixed, name))
            for g, rows, byte_idx in groups:
                a = getattr(g, name)
                if kind == "bytes":
                    full[byte_idx] = a
                else:
                    w = {"us": 48, "vs": 32}.get(name, 1)
                    full.reshape(-1, w)[rows] = a.reshape(-1, w)
            outs.append(full)
        return outs

    ENC_KINDS = [("rows", "us"), ("rows", "vs"), ("bytes", "ws"), ("rows", "ok")]
    DEC_KINDS = [("bytes", "out"), ("rows", "dok"), ("rows", "cls")]
    res_a = {}
    stats0 = (eng.tauth_lat_stats(), eng.tlock_stats(), eng.tlock_seal_stats())
    for mode, (o, s) in (("switch_off", (0, 0)), ("switch_on_1024_512", LAT_ON)):
        eng.set_tauth_lat_max(o, s)
        res_a["decrypt_" + mode] = compare(
            [("decrypt_auth", g.dec_uniform) for g, _, _ in groups], [("decrypt_auth_var", mixed.dec_var)],
            lambda: gathered(None, DEC_KINDS), lambda: list(mixed.dec_outputs()),
            lambda: bool(mixed.dok.min() == 1 and np.array_equal(mixed.out, mixed.msgs)), "a decrypt " + mode)
        res_a["encrypt_" + mode] = compare(
            [("encrypt_auth", g.enc_uniform) for g, _, _ in groups], [("encrypt_auth_var", mixed.enc_var)],
            lambda: gathered(None, ENC_KINDS), lambda: list(mixed.enc_outputs()),
            lambda: bool(mixed.ok.min() == 1), "a encrypt " + mode)
    eng.set_tauth_lat_max(0, 0)
    stats1 = (eng.tauth_lat_stats(), eng.tlock_stats(), eng.tlock_seal_stats())

    # ---- b1: a uniform 32 bytes through both entries (two Sets over the same inputs, so the outputs can be compared)
    u_var, u_uni = Set(np.full(N, UNIFORM, dtype=np.uint32)), Set(np.full(N, UNIFORM, dtype=np.uint32))
    u_uni.msgs[:] = u_var.msgs
    check(u_var.enc_var(), "encrypt_auth_var")
    u_uni.take_ciphertexts(u_var)
    res_b1 = {
        "decrypt": compare([("decrypt_auth_var", u_var.dec_var)], [("decrypt_auth", u_uni.dec_uniform)],
                           lambda: list(u_var.dec_outputs()), lambda: list(u_uni.dec_outputs()),
                           lambda: bool(u_var.dok.min() == 1 and np.array_equal(u_var.out, u_var.msgs)), "b1 decrypt"),
        "encrypt": compare([("encrypt_auth_var", u_var.enc_var)], [("encrypt_auth", u_uni.enc_uniform)],
                           lambda: list(u_var.enc_outputs()), lambda: list(u_uni.enc_outputs()),
                           lambda: bool(u_var.ok.min() == 1), "b1 encrypt")}

    # ---- b2: the mixed call against a uniform call of the same count and (nearly) the same bytes
    same_bytes = Set(np.full(N, SAME_BYTES_MLEN, dtype=np.uint32))
    check(same_bytes.enc_uniform(), "encrypt_auth")
    res_b2 = {
        "mixed_total_bytes": mixed.total, "uniform_total_bytes": same_bytes.total,
        "decrypt": compare([("decrypt_auth_var", mixed.dec_var)], [("decrypt_auth", same_bytes.dec_uniform)],
                           lambda: None, lambda: None,
                           lambda: bool(mixed.dok.min() == 1 and same_bytes.dok.min() == 1), "b2 decrypt"),
        "encrypt": compare([("encrypt_auth_var", mixed.enc_var)], [("encrypt_auth", same_bytes.enc_uniform)],
                           lambda: None, lambda: None,
                           lambda: bool(mixed.ok.min() == 1 and same_bytes.ok.min() == 1), "b2 encrypt")}

    res = {"tool": "tools/tauth_var_bench.py", "device": torch.cuda.get_device_name(0), "items": N,
           "distinct_lengths": len(groups), "warmup_pairs": args.warmup,
           "timing": "host clock around the host-form call(s) of a side; the sides alternate call by call; medians of "
                     "the pairs after the warm-up; a_over_b = side a's median over side b's",
           "prediction_written_before_the_run": PREDICTION,
           "a_per_length_calls_as_a_one_var_call_as_b": res_a,
           "b1_uniform_32_var_entry_as_a_uniform_entry_as_b": res_b1,
           "b2_mixed_var_as_a_uniform_same_bytes_as_b": res_b2,
           "same_bytes_ok_and_classes_in_every_pair": state["same"], "all_good": state["good"],
           "tauth_lat_stats_moved_by_in_a": [y - x for x, y in zip(stats0[0], stats1[0])],
           "tlock_stats_moved_by_in_a": [y - x for x, y in zip(stats0[1], stats1[1])],
           "tlock_seal_stats_moved_by_in_a": [y - x for x, y in zip(stats0[2], stats1[2])]}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    path = args.out or (os.path.join(ROOT, "profiles", "tauth_var_bench.json") if on_mi355x else None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if state["same"] and state["good"] else 1


if __name__ == "__main__":
    sys.exit(main())
