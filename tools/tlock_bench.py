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
    args = ap.parse_args()
    if args.sealed:
        return sealed(args)

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
