#!/usr/bin/env python3
"""Timelock opening against the exact verification step on one MI355X (not part of bench.py: no
headline number comes from here).

One context. --items device-resident compressed U values under one round signature (the golden chain's
round-7 SignatureV2; --distinct different points (i + 1) * G1, tiled) and one device-generated chained
history of the same length (the bench workload). After warm-up, --pairs interleaved pairs of
Engine.verify_chained_dev and Engine.tlock_open_dev, each timed with a host clock around the call and
a device synchronise; then one more pair with the stage events on (Engine.profile_read) for the
per-stage split. The yardstick: the opening's tlock + final_exp stage time against the SAME
run's exact miller + final_exp time, beside the ratio the host-build Fp-product counts predict
(profiles/tlock_opcount.json, profiles/opcount.json). Also the fixed cost a small call pays: a
one-item call with a new signature (decode + prepare + one pass) and with the cached one.

    python tools/tlock_bench.py --out profiles/tlock_bench.json

--sealed measures the producing side instead (see sealed() below): distinct scalars sealed on the device,
the result opened, every opened value compared with the sealed one.

    python tools/tlock_bench.py --sealed            # writes profiles/tseal_bench.json on an MI355X

--sealed-rounds measures the sealing to many rounds (see sealed_rounds() below): distinct scalars to
distinct rounds in one call beside the one-round seal and the opening, the 64-round fixed-cost case and
the crossover against a loop of one-round seals.

    python tools/tlock_bench.py --sealed-rounds     # writes profiles/tseal_rounds_bench.json on an MI355X
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def consecutive_points(n):
    """compress((i + 1) * G1), i < n: Jacobian mixed additions and one inversion for all of them."""
    from oracle import bls12381 as O
    p = O.P
    x2, y2 = O.G1
    two = O.g1_add(O.G1, O.G1)
    jac = [(x2, y2, 1), (two[0], two[1], 1)][:n]
    while len(jac) < n:
        x1, y1, z1 = jac[-1]
        zz = z1 * z1 % p
        h = (x2 * zz - x1) % p
        r = (y2 * z1 * zz - y1) % p
        hh = h * h % p
        hhh = h * hh % p
        v = x1 * hh % p
        x3 = (r * r - hhh - 2 * v) % p
        jac.append((x3, (r * (v - x3) - y1 * hhh) % p, z1 * h % p))
    pre, acc = [], 1
    for _, _, z in jac:
        pre.append(acc)
        acc = acc * z % p
    inv = O.fp_inv(acc)
    out = [None] * n
    for k in range(n - 1, -1, -1):
        x, y, z = jac[k]
        zi = inv * pre[k] % p
        inv = inv * z % p
        out[k] = O.g1_compress((x * zi * zi % p, y * zi * zi * zi % p))
    return out


def sealed(args):
    """--sealed: n DISTINCT seeded scalars sealed on the device (Engine.tlock_seal_dev) to the golden
    chain's round 7 under its key, and the resulting U values opened with that round's SignatureV2
    (Engine.tlock_open_dev). One device comparison checks that every opened value is the sealed K. After
    warm-up, --pairs interleaved (seal, open) pairs, each timed with a host clock around the call and a
    device synchronise; medians. Also the fixed cost of a new base (a one-item seal to a new round
    against one to the cached round)."""
    import torch

    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tlock_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    sig = {b["round"]: bytes.fromhex(b["sig_v2"]) for b in ch["beacons"]}
    dev = torch.device("cuda", 0)
    n, round_ = args.items, 7
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    scalars = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=gen)
    us = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    ks = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    opened = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def seal(r=round_, m=n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.tlock_seal_dev(r, scalars.data_ptr(), m, us.data_ptr(), ks.data_ptr(), ok.data_ptr())
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def opening():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.tlock_open_dev(sig[round_], us.data_ptr(), n, opened.data_ptr(), cls.data_ptr())
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        seal()
        opening()
    seal_ms, open_ms = [], []
    for _ in range(args.pairs):
        seal_ms.append(seal())
        open_ms.append(opening())
    all_sealed = int(ok.min().item()) == 1 and int(cls.max().item()) == 0
    round_trip = bool(torch.equal(opened, ks))
    distinct_us = int(torch.unique(us.view(n, 48), dim=0).shape[0])
    eng.profile(True)
    eng.profile_read()
    seal()
    st_seal = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
    eng.profile(False)
    n1_new, n1_cached = [], []
    for k in range(args.pairs):
        n1_new.append(seal(100 + k, 1))
        n1_cached.append(seal(100 + k, 1))
    ms, mo = statistics.median(seal_ms), statistics.median(open_ms)
    counts = json.load(open(os.path.join(ROOT, "profiles", "tseal_opcount.json")))["fp_mul"]
    opening_counts = json.load(open(os.path.join(ROOT, "profiles", "tlock_opcount.json")))["fp_mul"]
    res = {"tool": "tools/tlock_bench.py --sealed", "items": n, "distinct_scalars": n, "distinct_us": distinct_us,
           "pairs": args.pairs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "timing": "host clock around the call and a device synchronise; device-resident inputs and outputs",
           "seal_ms": [round(x, 2) for x in seal_ms], "open_ms": [round(x, 2) for x in open_ms],
           "seal_ms_median": round(ms, 2), "open_ms_median": round(mo, 2),
           "seals_per_s": round(n / (ms / 1e3)), "opens_per_s": round(n / (mo / 1e3)),
           "seal_over_open_measured": round(ms / mo, 3),
           "seal_over_open_predicted_by_fp_products": round(
               (counts["u_fixed"] + counts["gt_fixed"]) / (opening_counts["tlock_f"] + opening_counts["final_exp"]), 3),
           "stage_ms_seal": st_seal,
           "seal_n1_new_base_ms_median": round(statistics.median(n1_new), 3),
           "seal_n1_cached_base_ms_median": round(statistics.median(n1_cached), 3),
           "all_sealed": all_sealed, "open_equals_sealed_k": round_trip,
           "tlock_seal_stats": eng.tlock_seal_stats(), "tlock_stats": eng.tlock_stats()}
    # an MI355X reports itself by its architecture; the device name can be a generic one
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out = args.out or (os.path.join(ROOT, "profiles", "tseal_bench.json") if on_mi355x else None)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if all_sealed and round_trip and distinct_us == n else 1


def sealed_rounds(args):
    """--sealed-rounds: n DISTINCT seeded scalars sealed on the device to n DISTINCT rounds 1..n in one
    call (Engine.tlock_seal_rounds_dev); beside it, in the same run, the same scalars sealed to the one
    round 7 (Engine.tlock_seal_dev) and the U values opened with round 7's SignatureV2
    (Engine.tlock_open_dev). After warm-up, --pairs interleaved repetitions of the three, each timed with
    a host clock around the call and a device synchronise; medians, and the stage events of one more
    many-rounds call. Device comparisons: both paths give the same U; the many-rounds call with every
    round set to 7 gives exactly the opened values; item 6 of the timed call (round 7) does too.

    The fixed-cost case the call exists for: 64 items with 64 distinct rounds as ONE call against 64
    one-item Engine.tlock_seal_dev calls (each builds a new base), interleaved, new rounds every
    repetition; the one call must be at least 10 times faster (exit status 1 otherwise), and both give the
    same bytes. The crossover: 4 rounds with m items each as one many-rounds call against 4 one-round
    calls, m in powers of 4: the smallest m at which the loop over the rounds wins."""
    import torch

    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tlock_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    sig = {b["round"]: bytes.fromhex(b["sig_v2"]) for b in ch["beacons"]}
    dev = torch.device("cuda", 0)
    n, round_ = args.items, 7
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    scalars = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=gen)
    rounds = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
    us_r = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    ks_r = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    ok_r = torch.empty(n, dtype=torch.uint8, device=dev)
    us = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    ks = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    opened = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def timed(f):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        f()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def seal_rounds(rs=rounds, m=n, at=0):
        return timed(lambda: eng.tlock_seal_rounds_dev(rs.data_ptr(), scalars.data_ptr() + 32 * at, m,
                                                       us_r.data_ptr() + 48 * at, ks_r.data_ptr() + 576 * at,
                                                       ok_r.data_ptr() + at))

    def seal_one(r=round_, m=n, at=0):
        return timed(lambda: eng.tlock_seal_dev(r, scalars.data_ptr() + 32 * at, m, us.data_ptr() + 48 * at,
                                                ks.data_ptr() + 576 * at, ok.data_ptr() + at))

    def opening():
        return timed(lambda: eng.tlock_open_dev(sig[round_], us.data_ptr(), n, opened.data_ptr(), cls.data_ptr()))

    for _ in range(args.warmup):
        seal_rounds(), seal_one(), opening()
    rounds_ms, one_ms, open_ms = [], [], []
    for _ in range(args.pairs):
        rounds_ms.append(seal_rounds())
        one_ms.append(seal_one())
        open_ms.append(opening())
    all_sealed = int(ok_r.min().item()) == 1 and int(ok.min().item()) == 1 and int(cls.max().item()) == 0
    same_us = bool(torch.equal(us_r, us))
    one_equals_open = bool(torch.equal(opened, ks))
    item_round7 = bool(torch.equal(ks_r.view(n, 576)[round_ - 1], opened.view(n, 576)[round_ - 1])) if n >= round_ else True
    distinct_ks = int(torch.unique(ks_r.view(n, 576)[:min(n, 65536), :16], dim=0).shape[0])
    eng.profile(True)
    eng.profile_read()
    seal_rounds()
    st_rounds = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
    eng.profile(False)
    # every round 7: the many-rounds path must give exactly what the opening gave
    seal_rounds(torch.full((n,), round_, dtype=torch.int64, device=dev))
    rounds_equal_open = bool(torch.equal(ks_r, opened))

    # the fixed-cost case: 64 items, 64 distinct rounds
    m64 = min(64, n)
    call_ms, loop_ms, fixed_same = [], [], True
    for rep in range(args.pairs + args.warmup):
        r0 = 1000 + 64 * rep
        rs = torch.arange(r0, r0 + m64, dtype=torch.int64, device=dev)
        a = seal_rounds(rs, m64)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(m64):
            eng.tlock_seal_dev(r0 + i, scalars.data_ptr() + 32 * i, 1, us.data_ptr() + 48 * i, ks.data_ptr() + 576 * i,
                               ok.data_ptr() + i)
        eng.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        fixed_same &= bool(torch.equal(ks_r[:576 * m64], ks[:576 * m64]) and torch.equal(us_r[:48 * m64], us[:48 * m64]))
        if rep >= args.warmup:
            call_ms.append(a)
            loop_ms.append(b)
    fixed_ratio = statistics.median(loop_ms) / statistics.median(call_ms)

    # the crossover: R rounds x m items
    R, cross, table = 4, None, []
    m = 1
    while R * m <= n:
        rs = (torch.arange(R * m, dtype=torch.int64, device=dev) % R) + 5000
        a, b = [], []
        for rep in range(3):
            a.append(seal_rounds(rs, R * m))
            t = 0.0
            for j in range(R):
                t += seal_one(6000 + 8 * rep + j + 100 * len(table), m, j * m)
            b.append(t)
        table.append({"items_per_round": m, "one_call_ms": round(statistics.median(a), 3),
                      "loop_ms": round(statistics.median(b), 3)})
        if cross is None and statistics.median(b) < statistics.median(a):
            cross = m
        m *= 4

    mr, ms, mo = statistics.median(rounds_ms), statistics.median(one_ms), statistics.median(open_ms)
    counts = json.load(open(os.path.join(ROOT, "profiles", "tsealr_opcount.json")))
    hash_mul = json.load(open(os.path.join(ROOT, "profiles", "opcount.json")))["fp_mul"]["hash"]
    one_counts = json.load(open(os.path.join(ROOT, "profiles", "tseal_opcount.json")))["fp_mul"]
    opening_counts = json.load(open(os.path.join(ROOT, "profiles", "tlock_opcount.json")))["fp_mul"]
    per_item = counts["per_item_without_hash"] + hash_mul
    res = {"tool": "tools/tlock_bench.py --sealed-rounds", "items": n, "distinct_rounds": n, "distinct_scalars": n,
           "distinct_k_prefixes_of_first_64ki": distinct_ks, "pairs": args.pairs, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "timing": "host clock around the call and a device synchronise; device-resident inputs and outputs",
           "seal_rounds_ms": [round(x, 2) for x in rounds_ms], "seal_one_round_ms": [round(x, 2) for x in one_ms],
           "open_ms": [round(x, 2) for x in open_ms],
           "seal_rounds_ms_median": round(mr, 2), "seal_one_round_ms_median": round(ms, 2), "open_ms_median": round(mo, 2),
           "seals_per_s_many_rounds": round(n / (mr / 1e3)), "seals_per_s_one_round": round(n / (ms / 1e3)),
           "opens_per_s": round(n / (mo / 1e3)),
           "stage_ms_seal_rounds": st_rounds,
           "fp_products_per_item": {"many_rounds": per_item, "one_round": one_counts["u_fixed"] + one_counts["gt_fixed"],
                                    "opening": opening_counts["tlock_f"] + opening_counts["final_exp"]},
           "many_rounds_over_open_measured": round(mr / mo, 3),
           "many_rounds_over_open_predicted_by_fp_products": round(
               per_item / (opening_counts["tlock_f"] + opening_counts["final_exp"]), 3),
           "fixed_cost_64_rounds": {"items": m64, "one_call_ms": [round(x, 3) for x in call_ms],
                                    "loop_of_one_item_seals_ms": [round(x, 3) for x in loop_ms],
                                    "one_call_ms_median": round(statistics.median(call_ms), 3),
                                    "loop_ms_median": round(statistics.median(loop_ms), 3),
                                    "speedup": round(fixed_ratio, 2), "required": 10, "same_bytes": fixed_same},
           "crossover": {"rounds": R, "table": table, "loop_wins_from_items_per_round": cross},
           "all_sealed": all_sealed, "same_us_on_both_paths": same_us, "one_round_equals_open": one_equals_open,
           "round7_item_equals_open": item_round7, "all_round7_equals_open": rounds_equal_open,
           "tlock_seal_rounds_stats": eng.tlock_seal_rounds_stats(), "tlock_seal_stats": eng.tlock_seal_stats(),
           "tlock_stats": eng.tlock_stats()}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out = args.out or (os.path.join(ROOT, "profiles", "tseal_rounds_bench.json") if on_mi355x else None)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    good = (all_sealed and same_us and one_equals_open and item_round7 and rounds_equal_open and fixed_same
            and fixed_ratio >= 10)
    return 0 if good else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--seg", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sealed", action="store_true",
                    help="seal --items distinct scalars on the device and open the result (profiles/tseal_bench.json)")
    ap.add_argument("--sealed-rounds", action="store_true",
                    help="seal --items scalars to --items distinct rounds in one call, beside the one-round seal and "
                         "the opening (profiles/tseal_rounds_bench.json)")
    args = ap.parse_args()
    if args.sealed:
        return sealed(args)
    if args.sealed_rounds:
        return sealed_rounds(args)

    import numpy as np
    import torch

    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tlock_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    sig = {b["round"]: bytes.fromhex(b["sig_v2"]) for b in ch["beacons"]}
    dev = torch.device("cuda", 0)
    n, seg = args.items, args.seg
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))

    # the exact step's workload: a device-generated chained history
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    seeds = torch.randint(0, 256, (-(-n // seg) * 96,), dtype=torch.uint8, device=dev, generator=gen)
    sigs = torch.empty(n * 96, dtype=torch.uint8, device=dev)
    eng.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), 1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n)
    bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    fb = torch.empty(1, dtype=torch.int64, device=dev)

    # the opening's workload
    distinct = min(args.distinct, n)
    pts = np.frombuffer(b"".join(consecutive_points(distinct)), np.uint8).reshape(distinct, 48)
    us = torch.from_numpy(np.ascontiguousarray(np.tile(pts, (-(-n // distinct), 1))[:n])).to(dev).reshape(-1)
    out = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def exact():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.verify_chained_dev(1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n, bm.data_ptr(), fb.data_ptr(), None)
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def opening(s=sig[7], m=n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.tlock_open_dev(s, us.data_ptr(), m, out.data_ptr(), cls.data_ptr())
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        exact()
        opening()
    exact_ms, open_ms = [], []
    for _ in range(args.pairs):
        exact_ms.append(exact())
        open_ms.append(opening())
    all_valid = int(np.unpackbits(bm.cpu().numpy().view("uint8")).sum()) == n and int(cls.max().item()) == 0
    # every distinct point's value appears once per tile: the first and the last tile agree
    rows = out.view(n, 576)
    tiles_equal = bool(torch.equal(rows[:distinct], rows[(n // distinct - 1) * distinct:(n // distinct) * distinct])) \
        if n >= 2 * distinct else True

    eng.profile(True)
    eng.profile_read()
    exact()
    st_exact = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
    opening()
    st_open = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
    # the fixed cost: sigma's decode and preparation alone (n = 0 with a new signature)
    eng.tlock_open_dev(sig[8], us.data_ptr(), 0, out.data_ptr(), None)
    prepare_stage_ms = round(eng.profile_read()["tlock"][0], 3)
    eng.profile(False)
    n1_new, n1_cached = [], []
    for k in range(args.pairs):
        n1_new.append(opening(sig[9 + (k & 1)], 1))
        n1_cached.append(opening(sig[9 + (k & 1)], 1))

    frozen = json.load(open(os.path.join(ROOT, "profiles", "opcount.json")))["fp_mul"]
    mine = json.load(open(os.path.join(ROOT, "profiles", "tlock_opcount.json")))["fp_mul"]
    predicted = (mine["tlock_f"] + mine["final_exp"]) / (frozen["miller"] + frozen["final_exp"])
    measured = (st_open["tlock"] + st_open["final_exp"]) / (st_exact["miller"] + st_exact["final_exp"])
    mo, me = statistics.median(open_ms), statistics.median(exact_ms)
    res = {"tool": "tools/tlock_bench.py", "items": n, "distinct_points": distinct, "seg_len": seg, "pairs": args.pairs,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "exact_ms": [round(x, 2) for x in exact_ms], "open_ms": [round(x, 2) for x in open_ms],
           "exact_ms_median": round(me, 2), "open_ms_median": round(mo, 2),
           "ciphertexts_per_s": round(n / (mo / 1e3)), "beacons_per_s_exact": round(n / (me / 1e3)),
           "stage_ms_exact": st_exact, "stage_ms_open": st_open,
           "ratio_predicted_by_fp_products": round(predicted, 3), "ratio_measured": round(measured, 3),
           "prepare_stage_ms": prepare_stage_ms,
           "open_n1_new_sigma_ms_median": round(statistics.median(n1_new), 3),
           "open_n1_cached_sigma_ms_median": round(statistics.median(n1_cached), 3),
           "all_valid": all_valid, "tiles_equal": tiles_equal, "tlock_stats": eng.tlock_stats()}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if all_valid and tiles_equal else 1


if __name__ == "__main__":
    sys.exit(main())
