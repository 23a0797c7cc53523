#!/usr/bin/env python3
"""Timelock opening across many rounds on one MI355X (not part of bench.py: no headline number comes
from here). Everything is measured in ONE run, through the device-pointer forms, with a host clock around
the call and a device synchronise; after --warmup calls, --reps repetitions, medians.

Inputs: --items DISTINCT U values (distinct seeded scalars sealed on the device) and as many distinct
valid G2 points as round signatures (a device-generated chained history: the opening does not verify
them). Three measurements:

  sweep      the --items U values over m = 1, 1 Ki, 32 Ki and --items rounds (equal runs) in one
             blsv_tlock_open_rounds_dev call each, beside blsv_tlock_open_dev on the m = 1 inputs (the
             yardstick; the two must give the same bytes).
  loop       64 items of 64 distinct rounds in one call against the same as 64 blsv_tlock_open_dev calls
             (interleaved; both must give the same bytes).
  crossover  run lengths 1, 2, 4, ... 128 at --items items: every tile uniform (dense_min = 1) against
             every tile mixed (dense_min = SIZE_MAX), interleaved. The smallest run length at which uniform
             wins is what the default dense_min should be (null when it wins at none of them).

    python tools/topen_rounds_bench.py            # writes profiles/topen_rounds_bench.json on an MI355X
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

SIZE_MAX = 2 ** 64 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib
    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("topen_rounds_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    dev = torch.device("cuda", 0)
    n = args.items
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    lib, h = eng.lib, eng.handle

    # n distinct U values, n distinct G2 points
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    scalars = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=gen)
    us = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    scratch = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    eng.tlock_seal_dev(7, scalars.data_ptr(), n, us.data_ptr(), scratch.data_ptr(), ok.data_ptr())
    seeds = torch.randint(0, 256, (-(-n // 64) * 96,), dtype=torch.uint8, device=dev, generator=gen)
    d_sigs = torch.empty(n * 96, dtype=torch.uint8, device=dev)
    eng.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), 1, 64, seeds.data_ptr(), 32, d_sigs.data_ptr(), n)
    eng.synchronize()
    all_sealed = int(ok.min().item()) == 1
    sigs = np.ascontiguousarray(d_sigs.cpu().numpy())
    sig_ptr = sigs.ctypes.data_as(_lib.u8p)
    del d_sigs, seeds, scalars
    out = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    ref = scratch  # the one-signature path's bytes
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    scl = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def timed(f):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rc = f()
        eng.synchronize()
        if rc:
            raise SystemExit("call failed: %d" % rc)
        return (time.perf_counter() - t0) * 1e3

    def rounds_call(counts, items=n, dst=out):
        return timed(lambda: lib.blsv_tlock_open_rounds_dev(h, sig_ptr, counts.ctypes.data_as(_lib.u64p), len(counts),
                                                            us.data_ptr(), items, dst.data_ptr(), cls.data_ptr(),
                                                            scl.data_ptr(), None))

    def one_call(j=0, at=0, items=n, dst=ref):
        sig = (ctypes.c_uint8 * 96).from_buffer(sigs, 96 * j)
        return timed(lambda: lib.blsv_tlock_open_dev(h, sig, us.data_ptr() + 48 * at, items, dst.data_ptr() + 576 * at,
                                                     None, None))

    def equal_runs(m):
        counts = np.full(m, n // m, dtype=np.uint64)
        counts[: n % m] += 1
        return counts

    # ---- sweep over m, the yardstick beside it
    ms = sorted({1, min(1 << 10, n), min(1 << 15, n), n})
    plans = {m: equal_runs(m) for m in ms}
    for _ in range(args.warmup):
        one_call()
        for m in ms:
            rounds_call(plans[m])
    sweep_ms, yard_ms = {m: [] for m in ms}, []
    same_as_one = True
    for _ in range(args.reps):
        yard_ms.append(one_call())
        for m in ms:
            sweep_ms[m].append(rounds_call(plans[m]))
            if m == 1:
                same_as_one &= bool(torch.equal(out, ref))
    all_opened = int(cls.max().item()) == 0 and int(scl[:n].max().item()) == 0
    yard = statistics.median(yard_ms)
    sweep = [{"rounds": m, "items_per_round": n / m, "ms": [round(x, 2) for x in sweep_ms[m]],
              "ms_median": round(statistics.median(sweep_ms[m]), 2),
              "opens_per_s": round(n / (statistics.median(sweep_ms[m]) / 1e3))} for m in ms]

    print("sweep done", file=sys.stderr, flush=True)

    # ---- 64 items of 64 distinct rounds: one call against a loop of one-signature calls
    k64 = min(64, n)
    ones = np.ones(k64, dtype=np.uint64)
    call_ms, loop_ms, loop_same = [], [], True
    for rep in range(args.warmup + max(args.reps, 5)):
        a = rounds_call(ones, k64)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for j in range(k64):
            sig = (ctypes.c_uint8 * 96).from_buffer(sigs, 96 * j)
            rc = lib.blsv_tlock_open_dev(h, sig, us.data_ptr() + 48 * j, 1, ref.data_ptr() + 576 * j, None, None)
            if rc:
                raise SystemExit("call failed: %d" % rc)
        eng.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        loop_same &= bool(torch.equal(out[:576 * k64], ref[:576 * k64]))
        if rep >= args.warmup:
            call_ms.append(a)
            loop_ms.append(b)
    loop_ratio = statistics.median(loop_ms) / statistics.median(call_ms)

    # ---- crossover: all-uniform against all-mixed per run length
    table, cross, forms_same = [], None, True
    default_before = eng.set_tlock_dense_min(0)
    for L in (1, 2, 4, 8, 16, 32, 64, 128):
        if L > n:
            break
        counts = equal_runs(n // L)
        uni, mix = [], []
        for rep in range(args.warmup + args.reps):
            eng.set_tlock_dense_min(SIZE_MAX)
            b = rounds_call(counts, dst=ref)
            eng.set_tlock_dense_min(1)
            a = rounds_call(counts, dst=out)
            if rep == 0:
                forms_same &= bool(torch.equal(out, ref))
            if rep >= args.warmup:
                uni.append(a)
                mix.append(b)
        mu, mm = statistics.median(uni), statistics.median(mix)
        table.append({"run_length": L, "rounds": n // L, "uniform_ms": [round(x, 2) for x in uni],
                      "mixed_ms": [round(x, 2) for x in mix], "uniform_ms_median": round(mu, 2),
                      "mixed_ms_median": round(mm, 2)})
        if cross is None and mu < mm:
            cross = L
        print("run length %d: uniform %.1f ms, mixed %.1f ms" % (L, mu, mm), file=sys.stderr, flush=True)
    eng.set_tlock_dense_min(0)

    res = {"tool": "tools/topen_rounds_bench.py", "items": n, "distinct_us": n, "distinct_signatures": n,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "timing": "host clock around the call and a device synchronise; device-resident U values and outputs, "
                     "signatures and counts in host memory",
           "sweep": sweep,
           "yardstick_tlock_open_dev": {"ms": [round(x, 2) for x in yard_ms], "ms_median": round(yard, 2),
                                        "opens_per_s": round(n / (yard / 1e3))},
           "loop_against_one_call": {"items": k64, "rounds": k64, "one_call_ms": [round(x, 3) for x in call_ms],
                                     "loop_of_tlock_open_ms": [round(x, 3) for x in loop_ms],
                                     "one_call_ms_median": round(statistics.median(call_ms), 3),
                                     "loop_ms_median": round(statistics.median(loop_ms), 3),
                                     "speedup": round(loop_ratio, 2), "same_bytes": loop_same},
           "crossover": {"items": n, "table": table, "uniform_wins_from_run_length": cross,
                         "dense_min_default_in_this_build": default_before},
           "all_sealed": all_sealed, "all_opened": all_opened, "one_round_equals_tlock_open": same_as_one,
           "uniform_equals_mixed": forms_same,
           "tlock_open_rounds_stats": eng.tlock_open_rounds_stats(), "tlock_stats": eng.tlock_stats()}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    path = args.out or (os.path.join(ROOT, "profiles", "topen_rounds_bench.json") if on_mi355x else None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if all_sealed and all_opened and same_as_one and loop_same and forms_same else 1


if __name__ == "__main__":
    sys.exit(main())
