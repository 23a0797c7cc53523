#!/usr/bin/env python3
"""Randomized batch verification against the exact check on one MI355X (not part of bench.py: the
headline number stays the exact check).

One device-generated chained history (segments of --seg rounds, the bench workload). Per group size
and per history (all valid, one bad round, 0.1% bad rounds): after warm-up, --pairs interleaved pairs of
Engine.verify_chained_dev and Engine.verify_chained_rlc_dev on the same context and buffers, each
timed with a host clock around the call and a device synchronise; then one more pair with the stage
events on (Engine.profile_read) for the per-stage split. The verdict checksum of every timed step
(popcount of the bitmap and first_bad) is compared with the exact path's and printed.

    python tools/rlc_bench.py --out profiles/rlc_bench.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--seg", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--groups", default="64,256,1024")
    ap.add_argument("--histories", default="valid,one_bad,permille_bad")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("rlc_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    dev = torch.device("cuda", 0)
    n, seg = args.rounds, args.seg
    eng = Engine(0)
    eng.set_public_key(bytes.fromhex(ch["pk"]))
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    seeds = torch.randint(0, 256, (-(-n // seg) * 96,), dtype=torch.uint8, device=dev, generator=gen)
    sigs = torch.empty(n * 96, dtype=torch.uint8, device=dev)
    eng.generate_chained_dev(int(ch["sk"], 16).to_bytes(32, "big"), 1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n)
    torch.cuda.synchronize(dev)
    rows = sigs.view(n, 96)
    bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    fb = torch.empty(1, dtype=torch.int64, device=dev)

    def step(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(1, seg, seeds.data_ptr(), 32, sigs.data_ptr(), n, bm.data_ptr(), fb.data_ptr(), None)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) * 1e3
        pop = int(np.unpackbits(bm.cpu().numpy().view("uint8")).sum())
        return dt, (pop, int(fb.item()) & ((1 << 64) - 1))

    def corrupt(kind):
        """indices whose signature is replaced by the one 40 rounds earlier (a bad pairing)"""
        if kind == "valid":
            return []
        if kind == "one_bad":
            return [n // 2 + 7]
        g = torch.Generator()
        g.manual_seed(5)
        k = max(1, n // 1000)
        return sorted(set((torch.randperm(n - 64, generator=g)[:k] + 64).tolist()))

    results = []
    for kind in args.histories.split(","):
        idx = corrupt(kind)
        saved = None
        if idx:
            it = torch.tensor(idx, device=dev)
            saved = rows[it].clone()
            rows[it] = rows[it - 40].clone()
        for g in [int(x) for x in args.groups.split(",")]:
            prev_g = eng.set_rlc_group(g)
            try:
                for _ in range(args.warmup):
                    step(eng.verify_chained_dev)
                    step(eng.verify_chained_rlc_dev)
                s0 = eng.rlc_stats()
                exact_ms, rlc_ms, same = [], [], True
                for _ in range(args.pairs):
                    te, ce = step(eng.verify_chained_dev)
                    tr, cr = step(eng.verify_chained_rlc_dev)
                    exact_ms.append(te)
                    rlc_ms.append(tr)
                    same = same and ce == cr
                s1 = eng.rlc_stats()
                eng.profile(True)
                eng.profile_read()
                step(eng.verify_chained_dev)
                st_exact = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
                step(eng.verify_chained_rlc_dev)
                st_rlc = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
                eng.profile(False)
            finally:
                eng.set_rlc_group(prev_g)
            me, mr = statistics.median(exact_ms), statistics.median(rlc_ms)
            rec = {"history": kind, "bad_rounds": len(idx), "group": g,
                   "exact_ms": [round(x, 2) for x in exact_ms], "rlc_ms": [round(x, 2) for x in rlc_ms],
                   "exact_ms_median": round(me, 2), "rlc_ms_median": round(mr, 2), "speedup": round(me / mr, 3),
                   "checksum": {"popcount": ce[0], "first_bad": None if ce[1] == (1 << 64) - 1 else ce[1]},
                   "checksums_equal": same,
                   "rlc_stats_per_step": [(b - a) // args.pairs for a, b in zip(s0, s1)],
                   "stage_ms_exact": st_exact, "stage_ms_rlc": st_rlc}
            print(json.dumps(rec), flush=True)
            results.append(rec)
        if saved is not None:
            rows[it] = saved
    out = {"tool": "tools/rlc_bench.py", "rounds": n, "seg_len": seg, "pairs": args.pairs, "warmup": args.warmup,
           "rlc_wpe_env": os.environ.get("BLSV_RLC_WPE"), "device": torch.cuda.get_device_name(0),
           "all_checksums_equal": all(r["checksums_equal"] for r in results), "results": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "results"}))
    eng.close()
    return 0 if out["all_checksums_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
