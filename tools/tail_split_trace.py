#!/usr/bin/env python3
"""The Miller f pass and final-exponentiation dispatches of each pipeline pass in a rocprofv3
--kernel-trace CSV: how long k_miller_f ran, and for a split pass (verify.cpp pairing_check) where the
remainder's dispatch fell relative to the main one and to the main range's k_fexp_* dispatches.

    python3 tools/tail_split_trace.py rp_kernel_trace.csv      # one JSON object

Times in ms. A pass is delimited by its k_miller_lines dispatch.
"""
import csv
import json
import re
import sys


def short(name):
    m = re.search(r"blsk::(k_\w+)(<\d+>)?", name)
    return (m.group(1) + (m.group(2) or "")) if m else None


def main(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if k:
                rows.append((k, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Grid_Size_X"])))
    rows.sort(key=lambda r: r[1])
    passes, cur = [], None
    for r in rows:
        if r[0].startswith("k_miller_lines"):
            cur = {"t0": r[1], "f": [], "fexp": []}
            passes.append(cur)
        elif cur is not None and r[0] == "k_miller_f":
            cur["f"].append(r)
        elif cur is not None and r[0].startswith("k_fexp"):
            cur["fexp"].append(r)
    out = []
    for p in passes:
        ms = lambda t: round((t - p["t0"]) / 1e6, 3)
        fs = sorted(p["f"], key=lambda r: -r[3])  # the main dispatch has the larger grid
        rec = {"k_miller_f": [{"items": r[3], "start": ms(r[1]), "end": ms(r[2]), "ms": round((r[2] - r[1]) / 1e6, 3)}
                              for r in fs]}
        big = max(r[3] for r in p["fexp"] if r[0] == "k_fexp_easy")
        mainx = [r for r in p["fexp"] if r[3] >= big]  # the main range's grids: easy = items, tri ~ 3.05 items
        rec["main_fexp"] = {"start": ms(min(r[1] for r in mainx)), "end": ms(max(r[2] for r in mainx))}
        side = [r for r in p["fexp"] if r[3] < big]
        if side:
            rec["side_fexp"] = {"start": ms(min(r[1] for r in side)), "end": ms(max(r[2] for r in side))}
        if len(fs) == 2:
            rem = rec["k_miller_f"][1]
            rec["remainder_after_main_f"] = rem["start"] >= rec["k_miller_f"][0]["end"]
            rec["remainder_inside_main_fexp"] = rec["main_fexp"]["start"] <= rem["start"] <= rec["main_fexp"]["end"]
        rec["pass_ms"] = ms(max(r[2] for r in p["f"] + p["fexp"]))
        out.append(rec)
    print(json.dumps({"trace": path, "passes": out}, indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
