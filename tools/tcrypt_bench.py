#!/usr/bin/env python3
"""Timelock encrypt / decrypt in one call against the entry points they fuse, on one MI355X (not part of
bench.py: no headline number comes from here).

One context; the two modes of every comparison alternate call by call, --pairs pairs after --warmup, each
call timed with a host clock around it and a device synchronise; medians. Every step's outputs are hashed
(SHA-256) and its verdict bytes summed outside the timed region, and a sample of the fused outputs is
checked against the raw Gt bytes of the same step run through callers.kdf_sha256_ctr on the host.

  1. _dev forms, --items items, mlen = --mlen: tlock_decrypt_dev against tlock_open_dev and
     tlock_encrypt_dev against tlock_seal_dev on identical device-resident inputs.
  2. host forms, same size: blsv_tlock_decrypt against blsv_tlock_open alone (which still owes its KDF), both
     through the C ABI on flat buffers; and for --kdf-items items the end-to-end figure of the old path,
     callers.timelock_open with kdf_sha256_ctr in Python, beside callers.timelock_decrypt.
  3. latency: a lone decrypt and a lone encrypt with both latency switches on, against open / seal there.

    python tools/tcrypt_bench.py            # writes profiles/tcrypt_bench.json on an MI355X
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


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--mlen", type=int, default=32)
    ap.add_argument("--kdf-items", type=int, default=65536)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--lat-pairs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from drand_amd import _lib, callers
    from drand_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("tcrypt_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    sig = {b["round"]: bytes.fromhex(b["sig_v2"]) for b in ch["beacons"] if b.get("sig_v2")}
    pk = bytes.fromhex(ch["pk"])
    dev = torch.device("cuda", 0)
    n, mlen, round_ = args.items, args.mlen, 7
    eng = Engine(0)
    eng.set_public_key(pk)
    lib, h = eng.lib, eng.handle
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    scalars = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=gen)
    msgs = torch.randint(0, 256, (n * mlen,), dtype=torch.uint8, device=dev, generator=gen)
    us = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    gt = torch.empty(n * 576, dtype=torch.uint8, device=dev)
    out = torch.empty(n * mlen, dtype=torch.uint8, device=dev)
    us2 = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    flag = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    eng.tlock_seal_dev(round_, scalars.data_ptr(), n, us.data_ptr(), gt.data_ptr(), flag.data_ptr())
    eng.synchronize()

    def timed(f):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        f()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def digest(t):
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    def sample_ok(gt_t, in_t, out_t):
        """out == in XOR kdf(gt) on 1,024 items spread over the batch, on the host"""
        idx = list(range(0, n, max(1, n // 1024)))[:1024]
        g = gt_t.view(n, 576)[idx].cpu().numpy()
        a = in_t.view(n, mlen)[idx].cpu().numpy()
        b = out_t.view(n, mlen)[idx].cpu().numpy()
        return all(bytes(x ^ y for x, y in zip(a[k].tobytes(), callers.kdf_sha256_ctr(g[k].tobytes(), mlen))) == b[k].tobytes()
                   for k in range(len(idx)))

    # ---- 1. the _dev forms
    steps = {"open_dev": lambda: eng.tlock_open_dev(sig[round_], us.data_ptr(), n, gt.data_ptr(), flag.data_ptr()),
             "decrypt_dev": lambda: eng.tlock_decrypt_dev(sig[round_], us.data_ptr(), msgs.data_ptr(), mlen, n, out.data_ptr(),
                                                          flag.data_ptr()),
             "seal_dev": lambda: eng.tlock_seal_dev(round_, scalars.data_ptr(), n, us2.data_ptr(), gt.data_ptr(),
                                                    flag.data_ptr()),
             "encrypt_dev": lambda: eng.tlock_encrypt_dev(round_, scalars.data_ptr(), msgs.data_ptr(), mlen, n, us2.data_ptr(),
                                                          out.data_ptr(), flag.data_ptr())}
    dev_res = {}
    good = True
    for a, b in (("open_dev", "decrypt_dev"), ("seal_dev", "encrypt_dev")):
        ms = {a: [], b: []}
        sums = {a: [], b: []}
        for rep in range(args.warmup + args.pairs):
            for name in (a, b):
                t = timed(steps[name])
                res_t = gt if name in ("open_dev", "seal_dev") else out
                if rep >= args.warmup:
                    ms[name].append(round(t, 3))
                    sums[name].append({"sha256": digest(res_t), "verdict_sum": int(flag.sum(dtype=torch.int64).item())})
            good &= sample_ok(gt, msgs, out)  # gt: this pair's raw step, out: its fused step
        good &= all(s == sums[a][0] for s in sums[a]) and all(s == sums[b][0] for s in sums[b])
        dev_res[b + "_vs_" + a] = {a + "_ms": ms[a], b + "_ms": ms[b], a + "_ms_median": med(ms[a]),
                                   b + "_ms_median": med(ms[b]), "ratio": round(med(ms[b]) / med(ms[a]), 4),
                                   a + "_per_s": round(n / (med(ms[a]) / 1e3)), b + "_plaintexts_per_s": round(n / (med(ms[b]) / 1e3)),
                                   a + "_outputs": sums[a][0], b + "_outputs": sums[b][0]}
    eng.profile(True)
    stages = {}
    for name in ("open_dev", "decrypt_dev", "seal_dev", "encrypt_dev"):
        eng.profile_read()
        timed(steps[name])
        stages[name] = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
    eng.profile(False)

    # ---- 2. the host forms through the C ABI on flat buffers
    u8p = _lib.u8p
    h_us = us.cpu().numpy()
    h_cs = msgs.cpu().numpy()
    h_gt = np.empty(n * 576, np.uint8)
    h_out = np.empty(n * mlen, np.uint8)
    h_ok, h_cls = np.empty(n, np.uint8), np.empty(n, np.uint8)
    sc = ctypes.c_uint8()
    p = lambda arr: arr.ctypes.data_as(u8p)
    sigb = _lib.buf(sig[round_])

    def host_open():
        assert lib.blsv_tlock_open(h, sigb, p(h_us), n, p(h_gt), p(h_ok), p(h_cls), ctypes.cast(ctypes.byref(sc), u8p)) == 0

    def host_decrypt():
        assert lib.blsv_tlock_decrypt(h, sigb, p(h_us), p(h_cs), mlen, n, _lib.KDF_SHA256_CTR, p(h_out), p(h_ok), p(h_cls),
                                      ctypes.cast(ctypes.byref(sc), u8p)) == 0

    ho, hd, hsum = [], [], []
    for rep in range(args.warmup + args.pairs):
        a = timed(host_open)
        b = timed(host_decrypt)
        if rep >= args.warmup:
            ho.append(round(a, 3))
            hd.append(round(b, 3))
            hsum.append({"open_sha256": hashlib.sha256(h_gt.tobytes()).hexdigest(),
                         "decrypt_sha256": hashlib.sha256(h_out.tobytes()).hexdigest(), "verdict_sum": int(h_ok.sum())})
    good &= all(s == hsum[0] for s in hsum)
    good &= hsum[0]["decrypt_sha256"] == dev_res["decrypt_dev_vs_open_dev"]["decrypt_dev_outputs"]["sha256"]
    m = min(args.kdf_items, n)
    cts = [(h_us[48 * i:48 * i + 48].tobytes(), h_cs[mlen * i:mlen * i + mlen].tobytes()) for i in range(m)]
    old_ms, new_ms, same = [], [], True
    for rep in range(args.warmup + 3):
        t0 = time.perf_counter()
        old = callers.timelock_open(eng, round_, sig[round_], cts, callers.kdf_sha256_ctr, verify=False)
        t1 = time.perf_counter()
        new = callers.timelock_decrypt(eng, round_, sig[round_], cts, verify=False)
        t2 = time.perf_counter()
        same &= old == new
        if rep >= args.warmup:
            old_ms.append(round((t1 - t0) * 1e3, 2))
            new_ms.append(round((t2 - t1) * 1e3, 2))
    good &= same
    host_res = {"items": n, "open_ms": ho, "decrypt_ms": hd, "open_ms_median": med(ho), "decrypt_ms_median": med(hd),
                "ratio": round(med(hd) / med(ho), 4), "decrypt_plaintexts_per_s": round(n / (med(hd) / 1e3)),
                "open_gt_values_per_s": round(n / (med(ho) / 1e3)), "outputs": hsum[0],
                "bytes_down_per_item": {"open": 577, "decrypt": mlen + 1},
                "python_end_to_end": {"items": m, "timelock_open_with_python_kdf_ms": old_ms,
                                      "timelock_decrypt_ms": new_ms, "timelock_open_ms_median": med(old_ms),
                                      "timelock_decrypt_ms_median": med(new_ms),
                                      "plaintexts_per_s_old_path": round(m / (med(old_ms) / 1e3)),
                                      "plaintexts_per_s_fused": round(m / (med(new_ms) / 1e3)), "same_plaintexts": same}}

    # ---- 3. the latency path: one item, both switches on
    eng.set_tlock_lat_max(4)
    eng.set_tseal_lat_max(4)
    k1 = _lib.buf(scalars[:32].cpu().numpy().tobytes())
    o_us, o_gt, o_c, o_ok = _lib.out_buf(48), _lib.out_buf(576), _lib.out_buf(mlen), _lib.out_buf(1)

    def lat(which):
        if which == "open":
            return lib.blsv_tlock_open(h, sigb, p(h_us), 1, o_gt, o_ok, None, None)
        if which == "decrypt":
            return lib.blsv_tlock_decrypt(h, sigb, p(h_us), p(h_cs), mlen, 1, _lib.KDF_SHA256_CTR, o_c, o_ok, None, None)
        if which == "seal":
            return lib.blsv_tlock_seal(h, None, round_, k1, 1, o_us, o_gt, o_ok)
        return lib.blsv_tlock_encrypt(h, None, round_, k1, p(h_cs), mlen, 1, _lib.KDF_SHA256_CTR, o_us, o_c, o_ok)

    lat_res = {}
    for a, b in (("open", "decrypt"), ("seal", "encrypt")):
        ta, tb = [], []
        for rep in range(args.warmup + args.lat_pairs):
            x = timed(lambda: lat(a))
            raw = bytes(o_gt)
            y = timed(lambda: lat(b))
            good &= bytes(o_c) == bytes(i ^ j for i, j in zip(h_cs[:mlen].tobytes(), callers.kdf_sha256_ctr(raw, mlen)))
            if rep >= args.warmup:
                ta.append(x)
                tb.append(y)
        lat_res[b + "_vs_" + a] = {a + "_ms_median": med(ta), b + "_ms_median": med(tb),
                                   "difference_ms": round(med(tb) - med(ta), 3), "pairs": args.lat_pairs}
    lat_res["tlock_lat_stats"], lat_res["tseal_lat_stats"] = eng.tlock_lat_stats(), eng.tseal_lat_stats()
    eng.set_tlock_lat_max(0)
    eng.set_tseal_lat_max(0)

    res = {"tool": "tools/tcrypt_bench.py", "items": n, "mlen": mlen, "pairs": args.pairs, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "timing": "host clock around the call and a device synchronise; the two modes alternate call by call",
           "dev_forms": dev_res, "stage_ms": stages, "host_forms": host_res, "latency": lat_res,
           "fused_outputs_match_the_host_kdf_and_repeat": bool(good),
           "tlock_stats": eng.tlock_stats(), "tlock_seal_stats": eng.tlock_seal_stats()}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out_path = args.out or (os.path.join(ROOT, "profiles", "tcrypt_bench.json") if on_mi355x else None)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
