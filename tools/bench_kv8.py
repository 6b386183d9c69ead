"""fp16 against FP8 (e4m3) K / V cache, every comparison inside ONE process and one call (boxes differ by +-3 %):

  * tokens/s of greedy generations: 7B at -n 256 and -n 2048, mistral7b at -n 2048, 7b_16k over positions 8 K .. 16 K (the time of a
    16384-token generation minus the time of an 8192-token one), the formats interleaved, the better of two runs each;
  * the K / V stream's slope in ns per context position per layer, the way q4_build_transformer prices it (measure_kv_price): dispatch
    timestamps of the stand-alone attention launch at two context lengths, here inside the eager network at fusion level 1 (both formats then
    run the same sequence of launches around it);
  * the crossover: the position from which an FP8 token is faster, from the two per-token lines a + b * position fitted to the above;
  * the logit distance FP8 - fp16 on 7B over 32 forced positions (rms, max, greedy agreement), beside the fp16 path's own distance from the
    oracle's forward_f64 (CPU, minutes: --f64 computes it, --f64-cache keeps it in an .npy).

Writes profiles/kv8_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import shutil
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llama_cu_awq_amd import api, synth  # noqa: E402

PROMPT = [1, 2436, 385, 3686, 388, 1048, 22796, 118]   # bench.py's prompt
FORCED = [1] + [int(v) for v in np.random.default_rng(20240229).integers(3, 32000, size=31)]


def model_file(name, model_dir):
    path = os.path.join(model_dir, "llama2_q4_synth_%s_seed20240229.bin" % name)
    geom = synth.GEOMETRIES[name]
    if os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(geom):
        return path
    if name == "7b_16k":        # the 7B weights under a header with seq_len 16384
        shutil.copyfile(model_file("7b", model_dir), path)
        with open(path, "r+b") as f:
            f.seek(24)
            f.write(struct.pack("<i", geom[6]))
    else:
        synth.write_model(path, geom)
    return path


def best_seconds(t, n, runs=2):
    t.generate_ids(PROMPT, n)                                 # warm: captures the graphs of every bin
    out = [t.generate_ids(PROMPT, n) for _ in range(runs)]
    assert all(r[2] == out[0][2] for r in out)
    return min(r[3] for r in out), out[0][2]


def attention_us(t, pos):
    """average dispatch-to-end time of the attention launches of 8 eager tokens from `pos`"""
    t.generate_ids(PROMPT, pos)
    assert t.pos() == pos, (t.pos(), pos)
    return t.bench_in_network(2, tokens=8)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_bench.json"))
    ap.add_argument("--skip-16k", action="store_true")
    ap.add_argument("--f64", action="store_true", help="compute the oracle's forward_f64 logits of the 32 forced positions (CPU, minutes)")
    ap.add_argument("--f64-cache", default=None, help=".npy of those logits: read when it exists, written after --f64")
    ap.add_argument("--only-f64", action="store_true", help="no GPU: compute and cache the forward_f64 logits, then stop")
    args = ap.parse_args()
    res = {"tokens_per_s": {}, "kv_slope_ns_per_position_per_layer": {}, "logit_distance_7b": {}}

    f64 = None
    if args.f64_cache and os.path.exists(args.f64_cache):
        f64 = np.load(args.f64_cache)
    elif args.f64 or args.only_f64:
        import oracle
        m = oracle.Model(model_file("7b", args.model_dir))
        f64 = np.stack([m.forward_f64(tok, pos) for pos, tok in enumerate(FORCED)])
        m.close()
        if args.f64_cache:
            np.save(args.f64_cache, f64)
    if args.only_f64:
        return

    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    res["device"] = api.device_info()[0]

    def both(name):
        path = model_file(name, args.model_dir)
        return {kv: api.Transformer(path, kv=kv) for kv in ("fp16", "fp8")}

    # ---- tokens/s -----------------------------------------------------------------------------------------------------------------
    for name, lengths in (("7b", (256, 2048)), ("mistral7b", (2048,))):
        ts = both(name)
        for n in lengths:
            row = {}
            for kv, t in ts.items():
                secs, timed = best_seconds(t, n)
                row[kv] = round(timed / secs, 1)
            row["fp8_over_fp16"] = round(row["fp8"] / row["fp16"], 4)
            res["tokens_per_s"]["%s_n%d" % (name, n)] = row
            print(name, n, row, flush=True)
        if name == "7b":
            # ---- the slope at 7B's own context, and the logit distance
            L.q4_set_fusion(1)
            sl = {}
            for kv, t in ts.items():
                a, b = attention_us(t, 1024), attention_us(t, 2032)
                sl[kv] = {"us_at_1024": round(a, 3), "us_at_2032": round(b, 3), "ns_per_position": round((b - a) * 1e3 / (2032 - 1024), 4)}
            L.q4_set_fusion(5)
            sl["fp8_over_fp16"] = round(sl["fp8"]["ns_per_position"] / sl["fp16"]["ns_per_position"], 4)
            res["kv_slope_ns_per_position_per_layer"]["7b_1024_2032"] = sl
            print("slope 7b", sl, flush=True)
            logits = {}
            for kv, t in ts.items():
                t.reset(FORCED)
                rows = []
                for pos in range(len(FORCED)):
                    t.run_transformer(False)
                    api.synchronize()
                    rows.append(t.logits().astype(np.float64))
                logits[kv] = np.stack(rows)
            d = logits["fp8"] - logits["fp16"]
            dist = {"fp8_minus_fp16": {"rms": float(np.sqrt((d ** 2).mean())), "max": float(np.abs(d).max()),
                                      "greedy_agreement": float((logits["fp8"].argmax(1) == logits["fp16"].argmax(1)).mean())},
                    "logit_rms": float(np.sqrt((logits["fp16"] ** 2).mean()))}
            if f64 is not None:
                for kv in ("fp16", "fp8"):
                    e = logits[kv] - f64
                    dist["%s_minus_f64" % kv] = {"rms": float(np.sqrt((e ** 2).mean())), "max": float(np.abs(e).max()),
                                                 "greedy_agreement": float((logits[kv].argmax(1) == f64.argmax(1)).mean())}
            res["logit_distance_7b"] = dist
            print("logits", dist, flush=True)
        for t in ts.values():
            t.close()

    # ---- 16 K -----------------------------------------------------------------------------------------------------------------------
    if not args.skip_16k:
        ts = both("7b_16k")
        row, line = {}, {}
        for kv, t in ts.items():
            s8, n8 = best_seconds(t, 8192, runs=1)
            s16, n16 = best_seconds(t, 16384, runs=1)
            row[kv] = round((n16 - n8) / (s16 - s8), 1)
            # per-token time a + b * position: T(n) = a n + b n^2 / 2 at the two lengths
            b = (s16 / n16 - s8 / n8) * 2.0 / (n16 - n8)
            a = s8 / n8 - b * n8 / 2.0
            line[kv] = {"us_per_token_at_0": round(a * 1e6, 2), "ns_per_position_per_token": round(b * 1e9, 4), "ns_per_position_per_layer": round(b * 1e9 / 32, 4),
                        "tokens_per_s_n8192": round(n8 / s8, 1), "tokens_per_s_n16384": round(n16 / s16, 1)}
        row["fp8_over_fp16"] = round(row["fp8"] / row["fp16"], 4)
        res["tokens_per_s"]["7b_16k_positions_8192_16384"] = row
        res["per_token_line_7b_16k"] = line
        da = (line["fp8"]["us_per_token_at_0"] - line["fp16"]["us_per_token_at_0"]) * 1e3
        db = line["fp16"]["ns_per_position_per_token"] - line["fp8"]["ns_per_position_per_token"]
        res["crossover_position"] = int(da / db) if db > 0 and da > 0 else (0 if db > 0 else None)    # None: FP8 never faster; 0: faster from the start
        L.q4_set_fusion(1)
        sl = {}
        for kv, t in ts.items():
            a, b = attention_us(t, 8192), attention_us(t, 16000)
            sl[kv] = {"us_at_8192": round(a, 3), "us_at_16000": round(b, 3), "ns_per_position": round((b - a) * 1e3 / (16000 - 8192), 4)}
        L.q4_set_fusion(5)
        sl["fp8_over_fp16"] = round(sl["fp8"]["ns_per_position"] / sl["fp16"]["ns_per_position"], 4)
        res["kv_slope_ns_per_position_per_layer"]["7b_16k_8192_16000"] = sl
        print("16k", row, line, sl, "crossover", res["crossover_position"], flush=True)
        for t in ts.values():
            t.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
