#!/usr/bin/env python3
"""Signing on the latency path against the batch path on one MI355X (not part of bench.py: no headline number
comes from here). Everything is measured in ONE run through blsv_sign of one context, with a host clock around
the call (it returns when its outputs are written). Per shape, after --warmup rounds, every round makes four
calls -- mode off twice, mode on twice (blsv_set_sign_lat_max 0: the batch path, the parent's code; and on) --
so the two modes alternate and each is also timed twice in a row: the median of |first - second| of a mode is
its same-mode spread, known before any difference between the modes is quoted. Medians over --reps rounds. In
every round the four calls must return identical bytes, or the tool exits non-zero.

Inputs: the golden chain's key; 32-byte messages (sha256 of a counter), a new one per call.

  a  a lone blsv_sign of a 32-byte message
  b  the node's round: two messages in one call (its V1 and V2 partials), with a share index
  c  n = 1, 2, 16, 64, 256, 512, 1024, 2048, 4096: the first n at which the batch path is faster
  d  the lone verify of the same run (blsv_verify_messages of one of these signatures), for scale

The recommended blsv_set_sign_lat_max is the largest swept n at which the latency path still wins, rounded
down to a power of two -- and none when the lone latency-path call is not faster than the batch path by more
than the same-mode spread.

    python tools/sign_lat_bench.py            # writes profiles/sign_lat_bench.json on an MI355X
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

SWEEP = (1, 2, 16, 64, 256, 512, 1024, 2048, 4096)
NMAX = SWEEP[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=32, help="rounds of four calls per lone measurement")
    ap.add_argument("--sweep-reps", type=int, default=7, help="rounds of four calls per n of the sweep")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib
    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("sign_lat_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    lib, h = eng.lib, eng.handle
    sk32 = _lib.buf(int(ch["sk"], 16).to_bytes(32, "big"))

    # a pool of distinct 32-byte messages; call k of a shape signs n of them from a moving offset
    pool = np.frombuffer(b"".join(hashlib.sha256(b"sign_lat_bench %d" % i).digest() for i in range(2 * NMAX)),
                         dtype=np.uint8).copy()
    lens = np.full(NMAX, 32, dtype=np.uint32)

    def p8(a, off=0):
        return ctypes.cast(a.ctypes.data + off, _lib.u8p)

    def sign(at, n, index, out):
        t0 = time.perf_counter()
        rc = lib.blsv_sign(h, sk32, index, p8(pool, 32 * at), ctypes.cast(lens.ctypes.data, _lib.u32p), n, p8(out))
        dt = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SystemExit("blsv_sign failed: %d" % rc)
        return dt

    state = {"same": True}

    def rounds_of(n, index, reps, warmup):
        stride = 98 if index >= 0 else 96
        outs = [np.empty(stride * n, dtype=np.uint8) for _ in range(4)]
        t = [[], [], [], []]
        for k in range(warmup + reps):
            at = (k * n) % NMAX
            dts = []
            for j, mode in enumerate((0, 0, NMAX, NMAX)):
                eng.set_sign_lat_max(mode)
                dts.append(sign(at, n, index, outs[j]))
            state["same"] &= all(np.array_equal(outs[0], o) for o in outs[1:])
            if k >= warmup:
                for j in range(4):
                    t[j].append(dts[j])
        eng.set_sign_lat_max(0)
        mo, mn = statistics.median(t[0] + t[1]), statistics.median(t[2] + t[3])
        so = statistics.median(abs(a - b) for a, b in zip(t[0], t[1]))
        sn = statistics.median(abs(a - b) for a, b in zip(t[2], t[3]))
        return {"n": n, "off_ms_median": round(mo, 4), "on_ms_median": round(mn, 4), "off_over_on": round(mo / mn, 2),
                "off_ms_min": round(min(t[0] + t[1]), 4), "on_ms_min": round(min(t[2] + t[3]), 4),
                "off_same_mode_spread_ms": round(so, 4), "on_same_mode_spread_ms": round(sn, 4),
                "on_faster_beyond_spread": bool(mo - mn > max(so, sn)), "rounds": reps}

    lat0 = eng.sign_lat_stats()
    res_a = rounds_of(1, -1, args.reps, args.warmup)
    print("a", res_a, file=sys.stderr, flush=True)
    res_b = rounds_of(2, 3, args.reps, args.warmup)
    print("b", res_b, file=sys.stderr, flush=True)
    sweep, cross, last_win = [], None, None
    for n in SWEEP:
        r = rounds_of(n, -1, args.sweep_reps, 2)
        sweep.append(r)
        if cross is None and r["off_ms_median"] < r["on_ms_median"]:
            cross = n
        if cross is None and r["on_faster_beyond_spread"]:
            last_win = n
        print("c", r, file=sys.stderr, flush=True)
    lat1 = eng.sign_lat_stats()

    # d: the lone verify of one of these signatures (the latency engine's verification, its default cutover)
    sig = np.empty(96, dtype=np.uint8)
    sign(0, 1, -1, sig)
    bm, cls, fb = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8), ctypes.c_uint64()
    tv = []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        rc = lib.blsv_verify_messages(h, None, p8(pool), ctypes.cast(lens.ctypes.data, _lib.u32p), 1, p8(sig), p8(bm),
                                      ctypes.byref(fb), p8(cls))
        dt = (time.perf_counter() - t0) * 1e3
        if rc or not (bm[0] & 1):
            raise SystemExit("the signature did not verify: rc %d class %d" % (rc, cls[0]))
        if k >= args.warmup:
            tv.append(dt)
    res_d = {"ms_median": round(statistics.median(tv), 4), "ms_min": round(min(tv), 4), "calls": args.reps}
    print("d", res_d, file=sys.stderr, flush=True)

    lone_wins = res_a["on_faster_beyond_spread"]
    rec = (1 << (last_win.bit_length() - 1)) if lone_wins and last_win else None
    res = {"tool": "tools/sign_lat_bench.py", "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "timing": "host clock around blsv_sign (it returns with its outputs written); mode off = "
                     "blsv_set_sign_lat_max(0), the batch path; mode on = blsv_set_sign_lat_max(4096); per round "
                     "off, off, on, on; medians over both calls of a mode; a mode's spread is the median of "
                     "|first - second| of its two calls in a row",
           "a_lone_sign_32_bytes": res_a, "b_two_messages_with_index": res_b, "c_sweep": sweep,
           "c_first_n_batch_path_faster": cross, "c_largest_n_latency_path_wins": last_win,
           "d_lone_verify_for_scale": res_d,
           "lone_latency_call_faster_beyond_spread": lone_wins, "recommended_sign_lat_max": rec,
           "same_bytes_in_every_round": state["same"],
           "sign_lat_stats_moved_by": [lat1[0] - lat0[0], lat1[1] - lat0[1]]}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    path = args.out or (os.path.join(ROOT, "profiles", "sign_lat_bench.json") if on_mi355x else None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if state["same"] else 1


if __name__ == "__main__":
    sys.exit(main())
