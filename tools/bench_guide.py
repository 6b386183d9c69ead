"""What guided decoding (q4_set_guide, csrc/q4_guide.hip) costs: tokens/s of 7B -n 256 generations -- greedy and the CLI's default sampler
(-t 0.5 -p 0.6) -- with no guide, with a one-state guide that allows everything (the pure launch: its tokens must be those of "off"), with a table of
about 256 states compiled by guide.from_regex over the committed tokenizer, and with that table together with top_k = 40; plus, greedy only, no guide
and the one-state guide with the screened classifier switched off (q4_set_greedy_screen(0)): a guided greedy step gives the screen up, and this pair
shows the launch's cost without that loss.

Every configuration runs in a fresh child process under its own time limit (a child that fails or runs out of time is reported as such and nothing
more is started); a child warms up (graph captures), then times `--runs` generations and reports the best and the median. With --parent-lib (a
libllama2_q4.so built from the parent commit) the parent's build and this build's "off" alternate on the same box in the same call, two processes
each (parent, off, parent, off): the spread of the two parent runs against each other and that of the two off runs are both recorded, beside every
process's own best, median and worst generation.

Writes profiles/guide_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT = [1, 2436, 385, 3686, 388, 1048, 22796, 118]   # bench.py's prompt
SAMPLERS = {"greedy": (0.0, 0.9), "sampled_t0.5_p0.6": (0.5, 0.6)}
VARIANTS = ("off", "one_state_all_live", "regex_256_states", "regex_256_states_top_k40")
NO_SCREEN = ("off_no_screen", "one_state_all_live_no_screen")      # greedy only
# nineteen words of up to twelve letters, then any run of words; six '~' end the text (only then may EOS come, so a generation runs its length)
PATTERN = r"([A-Za-z]{1,12}[ ,]){19}[A-Za-z ,]*~{6}"


def child(args):
    import numpy as np
    from llama_cu_awq_amd import api, guide, synth
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
    if args.variant.endswith("_no_screen"):
        api.set_greedy_screen(0)
    t = api.Transformer(path, temperature=temperature, topp=topp, seed=20240229)
    vocab = t.config.vocab_size
    g, states = None, 0
    if args.variant.startswith("one_state_all_live"):
        g = api.Guide(np.zeros((1, vocab), dtype=np.uint16))
    elif args.variant.startswith("regex"):
        tk = api.Tokenizer(os.path.join(ROOT, "tests", "golden", "tokenizer.bin"), vocab)
        g = api.Guide(guide.from_regex(PATTERN, tk.pieces()))
        tk.close()
    if g is not None:
        states = g.n_states
        t.set_guide(g)
    if args.variant.endswith("top_k40"):
        t.set_sampling(top_k=40)
    for _ in range(2):
        t.generate_ids(PROMPT, args.ntok)
    rates = []
    for _ in range(args.runs):
        toks, tps, timed, secs = t.generate_ids(PROMPT, args.ntok)
        rates.append(timed / secs)
    rates.sort()
    out = {"tokens_per_s_best": round(rates[-1], 1), "tokens_per_s_median": round(rates[len(rates) // 2], 1), "tokens_per_s_worst": round(rates[0], 1),
           "timed_tokens": int(timed), "runs": args.runs,
           "distinct_tokens": len(set(toks.tolist())), "tokens_crc32": zlib.crc32(toks.tobytes()), "guide_states": states}
    if g is not None:
        st = t.guide_states(len(PROMPT) - 1, args.ntok - len(PROMPT) + 1)      # every generating step of the last run
        out["on_track"] = bool((st >= 0).all())
    t.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, sampler, variant, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sampler", sampler, "--variant", variant, "--model", args.model, "--ntok", str(args.ntok),
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit, run side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--sampler", default="greedy")
    ap.add_argument("--variant", default="off")
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"model": args.model, "ntok": args.ntok, "pattern": PATTERN, "tokens_per_s": {}}
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
            step(row, "parent_first", sampler, "off", lib=args.parent_lib)
        step(row, "off", sampler, "off")
        if args.parent_lib:
            step(row, "parent_second", sampler, "off", lib=args.parent_lib)
            step(row, "off_second", sampler, "off")
        for variant in VARIANTS[1:] + (NO_SCREEN if sampler == "greedy" else ()):
            step(row, variant, sampler, variant)
        off = row.get("off", {}).get("tokens_per_s_best")
        for name, r in row.items():
            if off and "tokens_per_s_best" in r and name != "off":
                r["us_per_token_over_off"] = round(1e6 / r["tokens_per_s_best"] - 1e6 / off, 2)
        if not failed and sampler == "greedy":
            a, b = (row[n]["tokens_per_s_best"] for n in NO_SCREEN)
            row[NO_SCREEN[1]]["us_per_token_over_off_no_screen"] = round(1e6 / b - 1e6 / a, 2)
        if not failed:
            row["one_state_all_live"]["tokens_equal_off"] = row["one_state_all_live"]["tokens_crc32"] == row["off"]["tokens_crc32"]
            failed = not row["one_state_all_live"]["tokens_equal_off"]
        if args.parent_lib and not failed:
            a, b = row["parent_first"]["tokens_per_s_best"], row["parent_second"]["tokens_per_s_best"]
            c, d = off, row["off_second"]["tokens_per_s_best"]
            row["off_vs_parent"] = {"parent_spread_pct": round(100.0 * abs(a - b) / max(a, b), 2), "off_spread_pct": round(100.0 * abs(c - d) / max(c, d), 2),
                                    "off_mean_minus_parent_mean_pct": round(100.0 * ((c + d) - (a + b)) / (a + b), 2)}
        res["tokens_per_s"][sampler] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
