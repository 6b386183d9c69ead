"""What the log-probability records (q4_set_logprobs) cost: tokens/s of 7B -n 256 generations -- greedy and the CLI's default sampler (-t 0.5 -p 0.6) --
with the records off and with K = 0, 5 and 20.

Every configuration runs in a fresh child process under its own time limit (a child that fails or runs out of time is reported as such, the
others still run); a child warms up (graph captures), then times `--runs` generations and reports the best and the median. "off" is the default
path: it must equal the parent commit's bench.py figure on the same box within the README's +-3 % box spread.

Writes profiles/logprobs_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT = [1, 2436, 385, 3686, 388, 1048, 22796, 118]   # bench.py's prompt
SAMPLERS = {"greedy": (0.0, 0.9), "sampled_t0.5_p0.6": (0.5, 0.6)}
KS = (-1, 0, 5, 20)


def child(args):
    from llama_cu_awq_amd import api, synth
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    path = os.path.join(args.model_dir, "llama2_q4_synth_%s_seed20240229.bin" % args.model)
    geom = synth.GEOMETRIES[args.model]
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(geom)):
        synth.write_model(path, geom)
    temperature, topp = SAMPLERS[args.sampler]
    t = api.Transformer(path, temperature=temperature, topp=topp, seed=20240229, logprobs=None if args.k < 0 else args.k)
    for _ in range(2):
        t.generate_ids(PROMPT, args.ntok)
    rates = []
    for _ in range(args.runs):
        toks, tps, timed, secs = t.generate_ids(PROMPT, args.ntok)
        rates.append(timed / secs)
    rates.sort()
    out = {"tokens_per_s_best": round(rates[-1], 1), "tokens_per_s_median": round(rates[len(rates) // 2], 1), "timed_tokens": int(timed), "runs": args.runs}
    if args.k >= 0:
        import numpy as np
        tlp = t.logprobs(0, timed + 1)[0]
        out["mean_token_logprob"] = round(float(np.mean(tlp[len(PROMPT) - 1:])), 4)      # (a sanity figure: finite, negative)
    t.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b")
    ap.add_argument("--ntok", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--sampler", default="greedy")
    ap.add_argument("--k", type=int, default=-1)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"model": args.model, "ntok": args.ntok, "tokens_per_s": {}}
    for sampler in SAMPLERS:
        row = {}
        for k in KS:
            name = "off" if k < 0 else "K%d" % k
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sampler", sampler, "--k", str(k), "--model", args.model, "--ntok", str(args.ntok),
                   "--runs", str(args.runs), "--model-dir", args.model_dir]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                row[name] = json.loads(lines[-1][7:]) if p.returncode == 0 and lines else {"error": "exit status %d" % p.returncode, "stderr": p.stderr[-400:]}
            except subprocess.TimeoutExpired:
                row[name] = {"error": "no result within %d s" % args.limit}
            print(sampler, name, row[name], flush=True)
            if "error" in row[name]:
                break            # (a child that failed on the GPU: start nothing more there)
        off = row.get("off", {}).get("tokens_per_s_best")
        for name, r in row.items():
            if off and "tokens_per_s_best" in r and name != "off":
                r["us_per_token_over_off"] = round(1e6 / r["tokens_per_s_best"] - 1e6 / off, 2)
        res["tokens_per_s"][sampler] = row
        if any("error" in r for r in row.values()):
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 1 if any("error" in r for row in res["tokens_per_s"].values() for r in row.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
