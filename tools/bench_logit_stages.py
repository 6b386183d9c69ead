"""Whether the step's host path moved when the logit stages went into one table (csrc/q4_step.hip), on one MI355X: tokens/s of 7B -n 256 generations
with --parent-lib (a libllama2_q4.so built from the parent commit) and this build's library side by side, `--rounds` (4) fresh processes each,
interleaved (who goes first alternates from round to round), in two configurations:

  greedy_off    temperature 0, no stage, no records: the flagship path (the table is only asked "is any stage on")
  sampled_all   -t 0.5 -p 0.6 with all four stages on: a guide, DRY, top-k 40 and typical-p / top-n-sigma / Mirostat

A configuration is unchanged when the median of this build's per-process medians lies inside [min, max] of the parent's. Every process is a fresh
child under its own time limit; after a child that fails or runs out of time nothing more is started. Writes profiles/logit_stages_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_adaptive import PROMPT, open_library      # noqa: E402  (bench.py's prompt; the library with a stream set)

CONFIGS = {"greedy_off": (0.0, 0.9), "sampled_all": (0.5, 0.6)}


def child(args):
    import numpy as np
    from llama_cu_awq_amd import synth
    api = open_library()
    path = os.path.join(args.model_dir, "llama2_q4_synth_%s_seed20240229.bin" % args.model)
    geom = synth.GEOMETRIES[args.model]
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(geom)):
        synth.write_model(path, geom)
    temperature, topp = CONFIGS[args.config]
    t = api.Transformer(path, temperature=temperature, topp=topp, seed=20240229)
    guide = None
    if args.config == "sampled_all":
        table = np.zeros((1, t.config.vocab_size), dtype=np.uint16)
        table[0, 1::2] = api.GUIDE_DEAD                        # even tokens only, and no EOS: every run has its 256 tokens
        table[0, 2] = api.GUIDE_DEAD
        guide = api.Guide(table)
        t.set_guide(guide)
        t.set_dry(multiplier=0.8, base=1.75, allowed_length=2, last_n=1024)
        t.set_sampling(top_k=40)
        t.set_adaptive(typical_p=0.9, top_n_sigma=1.5, mirostat_tau=5.0, mirostat_eta=0.1)
    for _ in range(2):
        t.generate_ids(PROMPT, args.ntok)
    rates = []
    for _ in range(args.runs):
        toks, tps, timed, secs = t.generate_ids(PROMPT, args.ntok)
        rates.append(timed / secs)
    rates.sort()
    t.close()
    if guide is not None:
        guide.close()
    print("RESULT " + json.dumps({"tokens_per_s_best": round(rates[-1], 1), "tokens_per_s_median": round(rates[len(rates) // 2], 1),
                                  "timed_tokens": int(timed), "runs": args.runs}), flush=True)


def run_child(args, config, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", config, "--model", args.model, "--ntok", str(args.ntok), "--runs", str(args.runs),
           "--model-dir", args.model_dir]
    env = dict(os.environ, Q4_LIB_OVERRIDE=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != "Q4_LIB_OVERRIDE"}
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=env)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        return json.loads(lines[-1][7:]) if p.returncode == 0 and lines else {"error": "exit status %d" % p.returncode, "stderr": p.stderr[-400:]}
    except subprocess.TimeoutExpired:
        return {"error": "no result within %d s" % args.limit}


def summary(row):
    p, o = ([r["tokens_per_s_median"] for r in row[k]] for k in ("parent", "this"))
    pm, om = round(statistics.median(p), 2), round(statistics.median(o), 2)
    return {"parent_min": min(p), "parent_median": pm, "parent_max": max(p), "this_min": min(o), "this_median": om, "this_max": max(o),
            "this_minus_parent_percent": round(100.0 * (om - pm) / pm, 3), "unchanged": min(p) <= om <= max(p)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit")
    ap.add_argument("--model", default="7b")
    ap.add_argument("--ntok", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=400, help="seconds per child (the first one writes the model file)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_stages_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="greedy_off")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    res = {"model": args.model, "ntok": args.ntok, "configs": {},
           "note": "per process: median and best of `runs` generations behind two warm-up generations. unchanged: this build's median of medians lies "
                   "inside the parent's [min, max] of the same session"}
    failed = False
    for config in CONFIGS:
        row = {"parent": [], "this": []}
        for i in range(args.rounds):
            pair = (("parent", args.parent_lib), ("this", None))
            for who, lib in (pair if i % 2 == 0 else pair[::-1]):      # who goes first alternates: neither always follows a warm device
                r = {"error": "not started"} if failed else run_child(args, config, lib)
                print(config, who, r, flush=True)
                failed = failed or "error" in r
                row[who].append(r)
        if not failed:
            row["summary"] = summary(row)
        res["configs"][config] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
