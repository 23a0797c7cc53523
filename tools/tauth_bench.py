#!/usr/bin/env python3
"""The authenticated timelock against its unauthenticated mirror, on one MI355X (not part of bench.py: no
headline number comes from here). tools/tcrypt_bench.py's method:

One context; the two modes of every comparison alternate call by call, --pairs pairs after --warmup, each call
timed with a host clock around it and a device synchronise; medians. Every step's outputs are hashed (SHA-256)
and its verdict bytes summed outside the timed region; 1,024 sampled authenticated ciphertexts are checked
against tests/support/tauth_ref.py on the host, and the decrypted messages against the inputs on the device.

  1. _dev forms, --items items, mlen = --mlen: tlock_decrypt_auth_dev against tlock_decrypt_dev and
     tlock_encrypt_auth_dev against tlock_encrypt_dev, each on device-resident inputs of its own kind.
  2. stage events of one call of each.
  3. --caller-items items: callers.timelock_decrypt_auth (no beacon verification) against
     callers.timelock_decrypt(verify=True).

The prediction is written down before the run and travels in the output.

    python tools/tauth_bench.py            # writes profiles/tauth_bench.json on an MI355X
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Written before the first run. tools/opcount tauth counts 653 Fp products per item in the open tail's check
# (the mean of 12 items: about 59 mixed additions of 11 and the comparison's 4) against the 5,117 + 7,657 the
# opening spends; the tlock stage does its 5,117 per item in 96.1 ms per 1 Mi items (profiles/tcrypt_bench.json).
PREDICTION = {
    "open_tail_fp_products_per_item": 653,
    "opening_fp_products_per_item": 5117 + 7657,
    "tlock_stage_ms_per_mi_items": 96.1,
    "predicted_open_tail_ms_per_mi_items": round(653 / 5117 * 96.1, 1),
    "predicted_decrypt_overhead": round(653 / 5117 * 96.1 / 291.9, 4),
    "predicted_encrypt_overhead": "about a dozen compressions and one 384-bit reduction per item: inside the spread",
}


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--mlen", type=int, default=32)
    ap.add_argument("--caller-items", type=int, default=65536)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from drand_amd import callers
    from drand_amd.engine import Engine
    from oracle import bls12381 as O
    from tests.support import tauth_ref as A
    from tests.support import tlock_ref as T

    if not torch.cuda.is_available():
        raise SystemExit("tauth_bench needs the GPU: nothing here is measured without one")
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        ch = json.load(f)["chained"]
    sig = {b["round"]: bytes.fromhex(b["sig_v2"]) for b in ch["beacons"] if b.get("sig_v2")}
    pk = bytes.fromhex(ch["pk"])
    dev = torch.device("cuda", 0)
    n, mlen, round_ = args.items, args.mlen, 7
    eng = Engine(0)
    eng.set_public_key(pk)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    rnd = lambda k: torch.randint(0, 256, (k,), dtype=torch.uint8, device=dev, generator=gen)
    new = lambda k: torch.empty(k, dtype=torch.uint8, device=dev)
    seeds, scalars, msgs = rnd(n * 32), rnd(n * 32), rnd(n * mlen)
    us, vs, ws, ok = new(n * 48), new(n * 32), new(n * mlen), new(n)  # the authenticated ciphertexts
    us1, cs1 = new(n * 48), new(n * mlen)  # the mirror's
    us2, vs2, out2 = new(n * 48), new(n * 32), new(n * mlen)  # what the timed steps write
    out, cls = new(n * mlen), new(n)
    torch.cuda.synchronize(dev)
    P = lambda t: t.data_ptr()
    eng.tlock_encrypt_auth_dev(round_, P(seeds), P(msgs), mlen, n, P(us), P(vs), P(ws), P(ok))
    eng.tlock_encrypt_dev(round_, P(scalars), P(msgs), mlen, n, P(us1), P(cs1), P(ok))
    eng.synchronize()

    def timed(f):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        f()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def digest(*ts):
        h = hashlib.sha256()
        for t in ts:
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()

    steps = {
        "decrypt_dev": (lambda: eng.tlock_decrypt_dev(sig[round_], P(us1), P(cs1), mlen, n, P(out), P(cls)), (out,), cls),
        "decrypt_auth_dev": (lambda: eng.tlock_decrypt_auth_dev(sig[round_], P(us), P(vs), P(ws), mlen, n, P(out), P(cls)),
                             (out,), cls),
        "encrypt_dev": (lambda: eng.tlock_encrypt_dev(round_, P(scalars), P(msgs), mlen, n, P(us2), P(out2), P(ok)),
                        (us2, out2), ok),
        "encrypt_auth_dev": (lambda: eng.tlock_encrypt_auth_dev(round_, P(seeds), P(msgs), mlen, n, P(us2), P(vs2), P(out2),
                                                                P(ok)), (us2, vs2, out2), ok),
    }
    good = True
    dev_res = {}
    for a, b in (("decrypt_dev", "decrypt_auth_dev"), ("encrypt_dev", "encrypt_auth_dev")):
        ms = {a: [], b: []}
        sums = {a: [], b: []}
        for rep in range(args.warmup + args.pairs):
            for name in (a, b):
                f, outs, flag = steps[name]
                t = timed(f)
                if name.startswith("decrypt"):  # both open to the messages, every item good
                    good &= bool(torch.equal(out, msgs)) and int(cls.sum(dtype=torch.int64).item()) == 0
                if rep >= args.warmup:
                    ms[name].append(round(t, 3))
                    sums[name].append({"sha256": digest(*outs), "verdict_sum": int(flag.sum(dtype=torch.int64).item())})
        good &= all(s == sums[a][0] for s in sums[a]) and all(s == sums[b][0] for s in sums[b])
        dev_res[b + "_vs_" + a] = {a + "_ms": ms[a], b + "_ms": ms[b], a + "_ms_median": med(ms[a]),
                                   b + "_ms_median": med(ms[b]), "ratio": round(med(ms[b]) / med(ms[a]), 4),
                                   "difference_ms": round(med(ms[b]) - med(ms[a]), 3),
                                   b + "_per_s": round(n / (med(ms[b]) / 1e3)), a + "_outputs": sums[a][0],
                                   b + "_outputs": sums[b][0]}
    good &= bool(torch.equal(us2, us)) and bool(torch.equal(vs2, vs)) and bool(torch.equal(out2, ws))

    # 1,024 sampled ciphertexts against the reference on the host (one oracle pairing for the base)
    fb = A.FixedBase(T.gt_base(O.g2_decompress(sig[round_], check_subgroup=False)))
    idx = list(range(0, n, max(1, n // 1024)))[:1024]
    pick = lambda t, k: t.view(n, k)[idx].cpu().numpy()
    hs, hm, hu, hv, hw = pick(seeds, 32), pick(msgs, mlen), pick(us, 48), pick(vs, 32), pick(ws, mlen)
    sample_ok = True
    for k in range(len(idx)):
        seed, msg = hs[k].tobytes(), hm[k].tobytes()
        kk = A.h3(seed, msg)
        v, w = A.seal_tail(seed, msg, T.encode_gt(fb.pow(kk)))
        sample_ok &= (A.u_of(kk), v, w) == (hu[k].tobytes(), hv[k].tobytes(), hw[k].tobytes())
    good &= sample_ok

    eng.profile(True)
    stages = {}
    for name in steps:
        eng.profile_read()
        timed(steps[name][0])
        stages[name] = {k: round(v[0], 3) for k, v in eng.profile_read().items() if v[1]}
    eng.profile(False)

    # callers: the authenticated decrypt with no beacon verification against decrypt + verification
    m = min(args.caller_items, n)
    col = lambda t, k: [bytes(r) for r in t.view(n, k)[:m].cpu().numpy()]
    cts_auth = list(zip(col(us, 48), col(vs, 32), col(ws, mlen)))
    cts = list(zip(col(us1, 48), col(cs1, mlen)))
    want = col(msgs, mlen)
    auth_ms, ver_ms, same = [], [], True
    for rep in range(args.warmup + 3):
        t0 = time.perf_counter()
        a = callers.timelock_decrypt_auth(eng, round_, sig[round_], cts_auth)
        t1 = time.perf_counter()
        b = callers.timelock_decrypt(eng, round_, sig[round_], cts, verify=True)
        t2 = time.perf_counter()
        same &= a == want and b == want
        if rep >= args.warmup:
            auth_ms.append(round((t1 - t0) * 1e3, 2))
            ver_ms.append(round((t2 - t1) * 1e3, 2))
    good &= same
    caller_res = {"items": m, "timelock_decrypt_auth_ms": auth_ms, "timelock_decrypt_verify_true_ms": ver_ms,
                  "timelock_decrypt_auth_ms_median": med(auth_ms), "timelock_decrypt_verify_true_ms_median": med(ver_ms),
                  "same_plaintexts": same}

    res = {"tool": "tools/tauth_bench.py", "items": n, "mlen": mlen, "pairs": args.pairs, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "timing": "host clock around the call and a device synchronise; the two modes alternate call by call",
           "prediction": PREDICTION, "dev_forms": dev_res, "stage_ms": stages, "callers": caller_res,
           "sampled_items_match_the_reference": bool(sample_ok), "outputs_repeat_and_open": bool(good),
           "not_measured": ["other message lengths", "the rounds forms", "concurrent callers"],
           "tlock_stats": eng.tlock_stats(), "tlock_seal_stats": eng.tlock_seal_stats()}
    on_mi355x = "gfx950" in getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out_path = args.out or (os.path.join(ROOT, "profiles", "tauth_bench.json") if on_mi355x else None)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
