#!/usr/bin/env python3
"""Timelock sealing on the latency path against the batch path on one MI355X (not part of bench.py: no
headline number comes from here). Everything is measured in ONE run through the HOST forms
(blsv_tlock_seal, blsv_tlock_seal_rounds) of one context, with a host clock around the call (a host form
returns when its outputs are written); the two modes -- blsv_set_tseal_lat_max 0 (off: the batch path, the
parent's code) and on -- alternate call by call; after --warmup pairs, medians over --reps pairs. In every
comparison the two modes must return identical bytes, or the tool exits non-zero.

Inputs: 4096 seeded 32-byte scalars under the golden chain's key; rounds are plain integers.

  a  a lone blsv_tlock_seal to a new round every call (the one-entry base cache of mode off never hits)
  b  a lone blsv_tlock_seal to the same round every call (mode off has its cache hit)
  c  one round, n = 1, 2, 4, ... 4096 (the base cached in mode off)
  d  64 items of 64 distinct rounds in one blsv_tlock_seal_rounds
  e  the crossovers: the smallest n of (c) at which mode off is faster, and the same sweep through
     blsv_tlock_seal_rounds (every item its own round) -- what blsv_set_tseal_lat_max should be given
     (null when mode off wins at none of them)

    python tools/tseal_lat_bench.py            # writes profiles/tseal_lat_bench.json on an MI355X
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

NMAX = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=48, help="pairs of calls per lone-seal measurement")
    ap.add_argument("--sweep-reps", type=int, default=7, help="pairs of calls per n of a sweep")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib
    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tseal_lat_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    lib, h = eng.lib, eng.handle

    rng = np.random.default_rng(5)
    scalars = np.ascontiguousarray(rng.integers(0, 256, NMAX * 32, dtype=np.uint8))
    rounds = np.ascontiguousarray((np.arange(NMAX, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(1000)))
    assert len(set(rounds.tolist())) == NMAX

    class Out:
        def __init__(self, n):
            self.us = np.empty(48 * n, dtype=np.uint8)
            self.gt = np.empty(576 * n, dtype=np.uint8)
            self.ok = np.empty(n, dtype=np.uint8)

        def same(self, o):
            return all(np.array_equal(a, b) for a, b in ((self.us, o.us), (self.gt, o.gt), (self.ok, o.ok)))

        def sealed(self):
            return bool(self.ok.min() == 1)

    def p8(a, off=0):
        return ctypes.cast(a.ctypes.data + off, _lib.u8p)

    def seal(rnd, at, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_seal(h, None, int(rnd), p8(scalars, 32 * at), n, p8(o.us), p8(o.gt), p8(o.ok))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_seal failed: %d" % rc)
        return dt

    def seal_rounds(at, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_seal_rounds(h, None, ctypes.cast(rounds.ctypes.data + 8 * at, _lib.u64p), p8(scalars, 32 * at),
                                        n, p8(o.us), p8(o.gt), p8(o.ok))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_seal_rounds failed: %d" % rc)
        return dt

    state = {"same": True, "sealed": True}

    def pairs(call, n, reps, warmup):
        """reps pairs (mode off, mode on) of call(k, out) after warmup pairs; every pair compared"""
        a, b = Out(n), Out(n)
        off, on = [], []
        for k in range(warmup + reps):
            eng.set_tseal_lat_max(0)
            t_off = call(k, a)
            eng.set_tseal_lat_max(NMAX)
            t_on = call(k, b)
            state["same"] &= a.same(b)
            state["sealed"] &= a.sealed()
            if k >= warmup:
                off.append(t_off)
                on.append(t_on)
        eng.set_tseal_lat_max(0)
        mo, mn = statistics.median(off), statistics.median(on)
        return {"off_ms_median": round(mo, 4), "on_ms_median": round(mn, 4), "off_over_on": round(mo / mn, 2),
                "off_ms_min": round(min(off), 4), "on_ms_min": round(min(on), 4), "pairs": reps}

    def sweep(call, tag):
        rows, cross = [], None
        n = 1
        while n <= NMAX:
            r = pairs(lambda k, o, n=n: call(n, o), n, args.sweep_reps, 2)
            r["n"] = n
            rows.append(r)
            if cross is None and r["off_ms_median"] < r["on_ms_median"]:
                cross = n
            print(tag, r, file=sys.stderr, flush=True)
            n *= 2
        return rows, cross

    lat0, s0, sr0 = eng.tseal_lat_stats(), eng.tlock_seal_stats(), eng.tlock_seal_rounds_stats()
    # a: round 2^32 + k in both calls of pair k. Mode on leaves the base cache alone, so the off call of
    # pair k finds the base of pair k - 1 there and builds its own
    res_a = pairs(lambda k, o: seal((1 << 32) + k, k % NMAX, 1, o), 1, args.reps, args.warmup)
    print("a", res_a, file=sys.stderr, flush=True)
    res_b = pairs(lambda k, o: seal(7, k % NMAX, 1, o), 1, args.reps, args.warmup)
    print("b", res_b, file=sys.stderr, flush=True)
    sweep_c, cross_c = sweep(lambda n, o: seal(7, 0, n, o), "c")
    res_d = pairs(lambda k, o: seal_rounds(64 * (k % 8), 64, o), 64, max(args.sweep_reps, 9), 2)
    print("d", res_d, file=sys.stderr, flush=True)
    sweep_r, cross_r = sweep(lambda n, o: seal_rounds(0, n, o), "e")
    lat1, s1, sr1 = eng.tseal_lat_stats(), eng.tlock_seal_stats(), eng.tlock_seal_rounds_stats()

    half = res_a["on_ms_median"] * 2 <= res_a["off_ms_median"] and res_d["on_ms_median"] * 2 <= res_d["off_ms_median"]
    below = res_b["on_ms_median"] < res_b["off_ms_median"] * 0.98
    crosses = [c for c in (cross_c, cross_r) if c is not None]
    res = {"tool": "tools/tseal_lat_bench.py", "device": torch.cuda.get_device_name(0), "distinct_scalars": NMAX,
           "warmup": args.warmup,
           "timing": "host clock around the host-form call (it returns with its outputs written); mode off = "
                     "blsv_set_tseal_lat_max(0), the batch path; mode on = blsv_set_tseal_lat_max(4096); the modes "
                     "alternate call by call; medians",
           "a_lone_seal_new_round_every_call": res_a, "b_lone_seal_same_round": res_b, "c_one_round_sweep": sweep_c,
           "d_64_items_of_64_rounds": res_d, "e_crossover_n_one_round": cross_c, "e_seal_rounds_sweep": sweep_r,
           "e_crossover_n_seal_rounds": cross_r,
           "acceptance_on_at_most_half_of_off_in_a_and_d": half,
           "acceptance_on_below_off_by_more_than_2_percent_in_b": below,
           # the last n at which mode on still wins both sweeps; no recommendation when an acceptance is missed
           "recommended_tseal_lat_max": ((min(crosses) // 2) if crosses else NMAX) if half and below else None,
           "same_bytes_in_every_pair": state["same"], "all_sealed": state["sealed"],
           "tseal_lat_stats_moved_by": [lat1[0] - lat0[0], lat1[1] - lat0[1]],
           "tlock_seal_stats_moved_by": [s1[0] - s0[0], s1[1] - s0[1]],
           "tlock_seal_rounds_stats_moved_by": [sr1[0] - sr0[0], sr1[1] - sr0[1]]}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    path = args.out or (os.path.join(ROOT, "profiles", "tseal_lat_bench.json") if on_mi355x else None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if state["same"] and state["sealed"] else 1


if __name__ == "__main__":
    sys.exit(main())
