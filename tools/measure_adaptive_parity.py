#!/usr/bin/env python3
"""How far the adaptive truncation launch's fp32 statistics lie from float64: the worst |kernel - float64| / max(1, |float64|) of T_s (top-n-sigma's
threshold), H (typical-p's entropy) and d* (its deviation threshold, against the interval of tiers float64 admits) over the op-level test cases of
tests/adaptive_ref.py -- every size, input and configuration tests/test_adaptive_gpu.py launches. The tests assert 4 x these figures.
    python tools/measure_adaptive_parity.py [--out profiles/adaptive_parity.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adaptive_ref as ref  # noqa: E402
from llama_cu_awq_amd import api as q4  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_parity.json"))
    args = ap.parse_args()
    L = q4.lib()
    q4.check(L.q4_set_device(0))
    s = C.c_void_p()
    q4.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    F = np.float32
    worst, where, bounded_worst = {}, {}, {}
    launches = 0
    for n in ref.SIZES:
        dl, dr = q4.DevBuf(nbytes=2 * n), q4.DevBuf(nbytes=4 * q4.ADAPTIVE_RECORD)
        mu, side, tokens, pos = q4.DevBuf(nbytes=32), q4.DevBuf(nbytes=4 * (n + 2)), q4.DevBuf(np.zeros(8, dtype=np.int32)), q4.DevBuf(np.zeros(1, dtype=np.int32))
        for name, x in ref.inputs(n):
            for cname, c, t in ref.CONFIGS:
                dl.put(x)
                mu.put(np.full(8, np.nan, dtype=F))
                q4.adaptive_mask(dl, n, temperature=t, mu_ring=mu, side=side, tokens=tokens, pos=pos, record=dr, **c)
                q4.synchronize()
                rec = q4.adaptive_record(dr.get(F, q4.ADAPTIVE_RECORD))
                _, dev, bounded, _ = ref.staged(x, rec, c, t, ref.Chain(), 0, None)
                launches += 1
                for k, v in dev.items():
                    if v >= worst.get(k, -1.0):
                        worst[k], where[k] = float(v), "n %d, %s, %s" % (n, name, cname)
                for k, g, w, tol in bounded:                   # (reported beside them: the share of its derived bound each quantity used)
                    bounded_worst[k] = max(bounded_worst.get(k, 0.0), float(abs(g - w) / tol))
    out = {"what": "worst |kernel - float64| / max(1, |float64|) over the op-level cases of tests/adaptive_ref.py; d_star against the interval of "
                   "tiers float64 admits at typical_p -+ eps", "launches": launches, "worst": worst, "where": where,
           "share_of_derived_bound": bounded_worst, "device": q4.device_info()[0]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    L.q4_set_stream(None)
    L.q4_stream_destroy(s)


if __name__ == "__main__":
    main()
