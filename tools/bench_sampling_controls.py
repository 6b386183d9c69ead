"""What the sampling controls (q4_sampler_set_controls / _set_logit_bias, csrc/q4_logit_process.hip) cost: tokens/s of 7B -n 256 generations -- greedy
and the CLI's default sampler (-t 0.5 -p 0.6) -- with the controls off, top-k 40 alone, penalties alone over a window of 64 and of 1024 ring entries,
and everything at once with 256 biases; plus, greedy only, the 1024-entry window on a generation long enough to fill it (-n 2048; at -n 256 a window
holds at most 256 entries).

Every configuration runs in a fresh child process under its own time limit (a child that fails or runs out of time is reported as such and nothing
more is started); a child warms up (graph captures), then times `--runs` generations and reports the best and the median. With --parent-lib (a
libllama2_q4.so built from the parent commit) the parent's build runs on the same box in the same call, once before and once after this build's
"off": "off" must equal the parent within the spread of the two parent runs against each other, and both are recorded.

Writes profiles/sampling_controls_bench.json (or --out)."""
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
PENALTIES = dict(repeat_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)
VARIANTS = {
    "off": None,
    "top_k40": dict(top_k=40),
    "penalties_last64": dict(penalty_last_n=64, **PENALTIES),
    "penalties_last1024": dict(penalty_last_n=1024, **PENALTIES),
    "everything_256_biases": dict(top_k=40, min_p=0.05, penalty_last_n=64, **PENALTIES),
}


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
    t = api.Transformer(path, temperature=temperature, topp=topp, seed=20240229)
    controls = VARIANTS[args.variant]
    if controls is not None:
        t.set_sampling(**controls)
        if args.variant == "everything_256_biases":      # small biases on ids 1000 .. 1255: the launch does the work, the text stays a text
            t.set_logit_bias({1000 + i: -0.25 for i in range(api.MAX_LOGIT_BIAS)})
    for _ in range(2):
        t.generate_ids(PROMPT, args.ntok)
    rates = []
    for _ in range(args.runs):
        toks, tps, timed, secs = t.generate_ids(PROMPT, args.ntok)
        rates.append(timed / secs)
    rates.sort()
    out = {"tokens_per_s_best": round(rates[-1], 1), "tokens_per_s_median": round(rates[len(rates) // 2], 1), "timed_tokens": int(timed), "runs": args.runs,
           "distinct_tokens": len(set(toks.tolist()))}
    t.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, sampler, variant, ntok, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sampler", sampler, "--variant", variant, "--model", args.model, "--ntok", str(ntok),
           "--runs", str(args.runs), "--model-dir", args.model_dir]
    env = dict(os.environ, Q4_LIB_OVERRIDE=os.path.abspath(lib)) if lib else os.environ
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=env)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        return json.loads(lines[-1][7:]) if p.returncode == 0 and lines else {"error": "exit status %d" % p.returncode, "stderr": p.stderr[-400:]}
    except subprocess.TimeoutExpired:
        return {"error": "no result within %d s" % args.limit}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b")
    ap.add_argument("--ntok", type=int, default=256)
    ap.add_argument("--long-ntok", type=int, default=2048, help="the generation that fills a 1024-entry window (0: leave it out)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit, run side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_controls_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--sampler", default="greedy")
    ap.add_argument("--variant", default="off")
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"model": args.model, "ntok": args.ntok, "tokens_per_s": {}}
    failed = False

    def step(row, name, *a, **kw):
        nonlocal failed
        if failed:               # (a child that failed on the GPU: start nothing more there)
            return
        row[name] = run_child(args, *a, **kw)
        print(name, row[name], flush=True)
        failed = "error" in row[name]

    for sampler in SAMPLERS:
        row = {}
        if args.parent_lib:
            step(row, "parent_first", sampler, "off", args.ntok, lib=args.parent_lib)
        step(row, "off", sampler, "off", args.ntok)
        if args.parent_lib:
            step(row, "parent_second", sampler, "off", args.ntok, lib=args.parent_lib)
        for variant in VARIANTS:
            if variant != "off":
                step(row, variant, sampler, variant, args.ntok)
        off = row.get("off", {}).get("tokens_per_s_best")
        for name, r in row.items():
            if off and "tokens_per_s_best" in r and name != "off":
                r["us_per_token_over_off"] = round(1e6 / r["tokens_per_s_best"] - 1e6 / off, 2)
        if args.parent_lib and not failed:
            a, b = row["parent_first"]["tokens_per_s_best"], row["parent_second"]["tokens_per_s_best"]
            row["off_vs_parent"] = {"parent_spread_pct": round(100.0 * abs(a - b) / max(a, b), 2),
                                    "off_minus_parent_mean_pct": round(100.0 * (off - 0.5 * (a + b)) / (0.5 * (a + b)), 2)}
        res["tokens_per_s"][sampler] = row
    if args.long_ntok and not failed:
        row = {}
        step(row, "off", "greedy", "off", args.long_ntok)
        step(row, "penalties_last1024", "greedy", "penalties_last1024", args.long_ntok)
        if not failed:
            row["penalties_last1024"]["us_per_token_over_off"] = round(1e6 / row["penalties_last1024"]["tokens_per_s_best"] - 1e6 / row["off"]["tokens_per_s_best"], 2)
        res["tokens_per_s"]["greedy_n%d" % args.long_ntok] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
