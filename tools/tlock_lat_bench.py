#!/usr/bin/env python3
"""Timelock opening on the latency path against the batch path on one MI355X (not part of bench.py: no
headline number comes from here). Everything is measured in ONE run through the HOST forms
(blsv_tlock_open, blsv_tlock_open_rounds), with a host clock around the call (a host form returns when its
outputs are written); the two modes -- blsv_set_tlock_lat_max 0 (off: the batch path, the parent's code)
and on -- alternate call by call; after --warmup pairs, medians over --reps pairs. In every comparison the
two modes must return identical bytes, or the tool exits non-zero.

Inputs: 4096 distinct U values (seeded scalars sealed on the device) and 64 distinct valid G2 points as
signatures (a device-generated chained history: the opening does not verify them).

  a  a lone blsv_tlock_open whose sigma changes every call (64 signatures in turn: the one-entry cache of
     mode off never hits)
  b  a lone blsv_tlock_open under the same sigma every call (mode off has its cache hit)
  c  one sigma, n = 1, 2, 4, ... 4096
  d  64 items of 64 distinct rounds in one blsv_tlock_open_rounds
  e  the crossover: the smallest n of (c) at which mode off is faster -- what blsv_set_tlock_lat_max
     should be given (null when mode off wins at none of them)

    python tools/tlock_lat_bench.py            # writes profiles/tlock_lat_bench.json on an MI355X
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

NSIG, NMAX = 64, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=64, help="pairs of calls per lone-open measurement")
    ap.add_argument("--sweep-reps", type=int, default=7, help="pairs of calls per n of the sweep")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib
    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tlock_lat_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    lib, h = eng.lib, eng.handle

    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    scalars = torch.randint(0, 256, (NMAX * 32,), dtype=torch.uint8, device=dev, generator=gen)
    d_us = torch.empty(NMAX * 48, dtype=torch.uint8, device=dev)
    d_gt = torch.empty(NMAX * 576, dtype=torch.uint8, device=dev)
    d_ok = torch.empty(NMAX, dtype=torch.uint8, device=dev)
    eng.tlock_seal_dev(7, scalars.data_ptr(), NMAX, d_us.data_ptr(), d_gt.data_ptr(), d_ok.data_ptr())
    seeds = torch.randint(0, 256, (96,), dtype=torch.uint8, device=dev, generator=gen)
    d_sigs = torch.empty(NSIG * 96, dtype=torch.uint8, device=dev)
    eng.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), 1, 64, seeds.data_ptr(), 32, d_sigs.data_ptr(), NSIG)
    eng.synchronize()
    all_sealed = int(d_ok.min().item()) == 1
    us = np.ascontiguousarray(d_us.cpu().numpy())
    sigs = np.ascontiguousarray(d_sigs.cpu().numpy())
    del scalars, d_us, d_gt, d_ok, seeds, d_sigs
    assert len({bytes(sigs[96 * j:96 * j + 96]) for j in range(NSIG)}) == NSIG

    class Out:
        def __init__(self, n, m):
            self.gt = np.empty(576 * n, dtype=np.uint8)
            self.ok = np.empty(n, dtype=np.uint8)
            self.cls = np.empty(n, dtype=np.uint8)
            self.sc = np.empty(m, dtype=np.uint8)

        def same(self, o):
            return all(np.array_equal(a, b) for a, b in ((self.gt, o.gt), (self.ok, o.ok), (self.cls, o.cls), (self.sc, o.sc)))

        def opened(self):
            return bool(self.ok.min() == 1 and self.sc.max() == 0)

    def p8(a, off=0):
        return ctypes.cast(a.ctypes.data + off, _lib.u8p)

    def open_one(j, at, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_open(h, p8(sigs, 96 * j), p8(us, 48 * at), n, p8(o.gt), p8(o.ok), p8(o.cls), p8(o.sc))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_open failed: %d" % rc)
        return dt

    def open_rounds(counts, n, o):
        t0 = time.perf_counter()
        rc = lib.blsv_tlock_open_rounds(h, p8(sigs), counts.ctypes.data_as(_lib.u64p), len(counts), p8(us), n, p8(o.gt),
                                        p8(o.ok), p8(o.cls), p8(o.sc))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_tlock_open_rounds failed: %d" % rc)
        return dt

    state = {"same": True, "opened": True}

    def pairs(call, n, m, reps, warmup):
        """reps pairs (mode off, mode on) of call(k, out) after warmup pairs; every pair compared"""
        a, b = Out(n, m), Out(n, m)
        off, on = [], []
        for k in range(warmup + reps):
            eng.set_tlock_lat_max(0)
            t_off = call(k, a)
            eng.set_tlock_lat_max(NMAX)
            t_on = call(k, b)
            state["same"] &= a.same(b)
            state["opened"] &= a.opened()
            if k >= warmup:
                off.append(t_off)
                on.append(t_on)
        eng.set_tlock_lat_max(0)
        mo, mn = statistics.median(off), statistics.median(on)
        return {"off_ms_median": round(mo, 4), "on_ms_median": round(mn, 4), "off_over_on": round(mo / mn, 2),
                "off_ms_min": round(min(off), 4), "on_ms_min": round(min(on), 4), "pairs": reps}

    lat0, tl0 = eng.tlock_lat_stats(), eng.tlock_stats()
    res_a = pairs(lambda k, o: open_one(k % NSIG, k % NMAX, 1, o), 1, 1, args.reps, args.warmup)
    print("a", res_a, file=sys.stderr, flush=True)
    res_b = pairs(lambda k, o: open_one(0, k % NMAX, 1, o), 1, 1, args.reps, args.warmup)
    print("b", res_b, file=sys.stderr, flush=True)
    sweep, cross = [], None
    n = 1
    while n <= NMAX:
        r = pairs(lambda k, o, n=n: open_one(0, 0, n, o), n, 1, args.sweep_reps, 2)
        r["n"] = n
        sweep.append(r)
        if cross is None and r["off_ms_median"] < r["on_ms_median"]:
            cross = n
        print("c", r, file=sys.stderr, flush=True)
        n *= 2
    ones = np.ones(NSIG, dtype=np.uint64)
    res_d = pairs(lambda k, o: open_rounds(ones, NSIG, o), NSIG, NSIG, max(args.sweep_reps, 9), 2)
    print("d", res_d, file=sys.stderr, flush=True)
    lat1, tl1 = eng.tlock_lat_stats(), eng.tlock_stats()

    factor2 = res_a["off_over_on"] >= 2.0 and res_b["off_over_on"] >= 2.0
    res = {"tool": "tools/tlock_lat_bench.py", "device": torch.cuda.get_device_name(0), "distinct_us": NMAX,
           "distinct_signatures": NSIG, "warmup": args.warmup,
           "timing": "host clock around the host-form call (it returns with its outputs written); mode off = "
                     "blsv_set_tlock_lat_max(0), the batch path; mode on = blsv_set_tlock_lat_max(4096); the modes "
                     "alternate call by call; medians",
           "a_lone_open_new_sigma_every_call": res_a, "b_lone_open_same_sigma": res_b, "c_one_sigma_sweep": sweep,
           "d_64_items_of_64_rounds": res_d, "e_crossover_n": cross,
           "acceptance_on_at_most_half_of_off_in_a_and_b": factor2,
           # the last n of the sweep at which mode on still wins; no recommendation when the factor is missed
           "recommended_tlock_lat_max": (NMAX if cross is None else cross // 2) if factor2 else None,
           "same_bytes_in_every_pair": state["same"], "all_sealed": all_sealed, "all_opened": state["opened"],
           "tlock_lat_stats_moved_by": [lat1[0] - lat0[0], lat1[1] - lat0[1]],
           "tlock_stats_moved_by": [tl1[0] - tl0[0], tl1[1] - tl0[1]]}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    path = args.out or (os.path.join(ROOT, "profiles", "tlock_lat_bench.json") if on_mi355x else None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if all_sealed and state["same"] and state["opened"] else 1


if __name__ == "__main__":
    sys.exit(main())
