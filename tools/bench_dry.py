"""What DRY and the no-repeat-n-gram ban (q4_sampler_set_dry, csrc/q4_dry.hip) cost, on one MI355X:

  tokens/s and microseconds per token of 7B -n 256 generations -- greedy and the CLI's default sampler (-t 0.5 -p 0.6) -- with everything off, DRY over
  a window of 1024 ring entries, the n-gram ban alone, and DRY in front of top-k 40; with --parent-lib (a libllama2_q4.so built from the parent commit)
  the parent and this build's "off" run side by side, `--rounds` (3) interleaved processes each: "unchanged" means the two medians differ by no more
  than the parent's own spread (max - min of its processes), which is recorded.

  greedy at -n 2048, where the windows fill: off, DRY over 1024 and over 4096 entries, and the sampling controls' penalties over 1024 entries -- the
  existing launch DRY's window-1024 cost is held against, measured again on the same machine in the same run.

  the launch alone (q4_dry_penalty / q4_process_logits on the q4 stream, host-timed over back-to-back calls, the same call on an empty window
  subtracted): the worst case, a window of one repeated token, at 1024 and 4096 entries; the penalties launch on the same 1024-entry window.

Every configuration runs in a fresh child process under its own time limit; a child that fails or runs out of time is reported as such and nothing
more is started. Writes profiles/dry_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT = [1, 2436, 385, 3686, 388, 1048, 22796, 118]   # bench.py's prompt
SAMPLERS = {"greedy": (0.0, 0.9), "sampled_t0.5_p0.6": (0.5, 0.6)}
DRY = dict(multiplier=0.8, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0)
PENALTIES = dict(repeat_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)
VARIANTS = {                                            # name: (dry, sampling)
    "off": (None, None),
    "dry_last1024": (DRY, None),
    "ngram4_only": (dict(DRY, multiplier=0.0, no_repeat_ngram_size=4), None),
    "dry_last1024_top_k40": (DRY, dict(top_k=40)),
    "dry_last4096": (dict(DRY, last_n=4096), None),
    "penalties_last1024": (None, dict(penalty_last_n=1024, **PENALTIES)),
}


def open_library():
    from llama_cu_awq_amd import api
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    return api


def child_tokens(args):
    from llama_cu_awq_amd import synth
    api = open_library()
    path = os.path.join(args.model_dir, "llama2_q4_synth_%s_seed20240229.bin" % args.model)
    geom = synth.GEOMETRIES[args.model]
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(geom)):
        synth.write_model(path, geom)
    temperature, topp = SAMPLERS[args.sampler]
    t = api.Transformer(path, temperature=temperature, topp=topp, seed=20240229)
    dry, sampling = VARIANTS[args.variant]
    if dry is not None:
        t.set_dry(**dry)
    if sampling is not None:
        t.set_sampling(**sampling)
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


def child_op(args):
    """microseconds per call over `--op-calls` back-to-back calls and one synchronise, best of five; `net`: minus the same call on an empty window"""
    import numpy as np
    api = open_library()
    n = 32000
    logits = api.DevBuf((np.random.default_rng(1).standard_normal(n) * 3.0).astype(np.float16))
    ring = api.DevBuf(np.zeros(8192, dtype=np.int32))          # one repeated token
    pos = {p: api.DevBuf(np.array([p], dtype=np.int32)) for p in (0, 5000)}

    def timed(call):
        call()
        api.synchronize()
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(args.op_calls):
                call()
            api.synchronize()
            dt = (time.perf_counter() - t0) / args.op_calls * 1e6
            best = dt if best is None else min(best, dt)
        return best

    out = {"calls": args.op_calls, "vocabulary": n}
    for name, ctl in (("dry_one_token_last1024", DRY), ("dry_one_token_last4096", dict(DRY, last_n=4096)),
                      ("ngram4_one_token_last4096", dict(DRY, multiplier=0.0, last_n=4096, no_repeat_ngram_size=4))):
        full = timed(lambda: api.dry_penalty(logits, n, tokens=ring, pos=pos[5000], **ctl))
        empty = timed(lambda: api.dry_penalty(logits, n, tokens=ring, pos=pos[0], **ctl))
        out[name] = {"us_per_call": round(full, 2), "us_per_call_empty_window": round(empty, 2), "us_net": round(full - empty, 2)}
    ctl = dict(penalty_last_n=1024, **PENALTIES)
    full = timed(lambda: api.process_logits(logits, n, tokens=ring, pos=pos[5000], **ctl))
    empty = timed(lambda: api.process_logits(logits, n, tokens=None, pos=None, **ctl))
    out["penalties_one_token_last1024"] = {"us_per_call": round(full, 2), "us_per_call_empty_window": round(empty, 2), "us_net": round(full - empty, 2)}
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, argv, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + argv + ["--model", args.model, "--runs", str(args.runs), "--model-dir", args.model_dir,
                                                                "--op-calls", str(args.op_calls)]
    env = dict(os.environ, Q4_LIB_OVERRIDE=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != "Q4_LIB_OVERRIDE"}
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
    ap.add_argument("--long-ntok", type=int, default=2048, help="the generation that fills the windows (0: leave it out)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved processes of the parent and of this build's off")
    ap.add_argument("--op-calls", type=int, default=200)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=400, help="seconds per child (the first one writes the model file)")
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit, run side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dry_bench.json"))
    ap.add_argument("--child", choices=("tokens", "op"), default=None)
    ap.add_argument("--sampler", default="greedy")
    ap.add_argument("--variant", default="off")
    args = ap.parse_args()
    if args.child == "tokens":
        return child_tokens(args)
    if args.child == "op":
        return child_op(args)
    res = {"model": args.model, "ntok": args.ntok, "tokens_per_s": {},
           "note": "us_per_token_over_off: 1e6 / tokens_per_s_best minus the same of this build's off (its best process). off_vs_parent: medians of the "
                   "per-process medians; unchanged = they differ by no more than parent_spread (max - min of the parent's processes). op: host-timed "
                   "back-to-back calls, each with its parameter upload; us_net subtracts the same call on an empty window"}
    failed = False

    def step(name, argv, **kw):
        nonlocal failed
        if failed:               # (a child that failed on the GPU: start nothing more there)
            return {"error": "not started"}
        r = run_child(args, argv, **kw)
        print(name, r, flush=True)
        failed = "error" in r
        return r

    def tokens(sampler, variant, ntok, lib=None):
        return step("%s %s n%d%s" % (sampler, variant, ntok, " (parent)" if lib else ""),
                    ["--child", "tokens", "--sampler", sampler, "--variant", variant, "--ntok", str(ntok)], lib=lib)

    def over_off(row):
        offs = [r["tokens_per_s_best"] for r in ([row.get("off")] if isinstance(row.get("off"), dict) else row.get("off", [])) if "tokens_per_s_best" in r]
        for name, r in row.items():
            if offs and isinstance(r, dict) and "tokens_per_s_best" in r and name != "off":
                r["us_per_token"] = round(1e6 / r["tokens_per_s_best"], 2)
                r["us_per_token_over_off"] = round(1e6 / r["tokens_per_s_best"] - 1e6 / max(offs), 2)

    for sampler in SAMPLERS:
        row = {"off": [], "parent": []}
        for _ in range(args.rounds):
            if args.parent_lib:
                row["parent"].append(tokens(sampler, "off", args.ntok, lib=args.parent_lib))
            row["off"].append(tokens(sampler, "off", args.ntok))
        for variant in ("dry_last1024", "ngram4_only", "dry_last1024_top_k40", "penalties_last1024"):
            row[variant] = tokens(sampler, variant, args.ntok)
        over_off(row)
        if args.parent_lib and not failed:
            med = lambda rs: sorted(r["tokens_per_s_median"] for r in rs)
            p, o = med(row["parent"]), med(row["off"])
            row["off_vs_parent"] = {"parent_median": p[len(p) // 2], "parent_spread": round(p[-1] - p[0], 1), "off_median": o[len(o) // 2],
                                    "off_spread": round(o[-1] - o[0], 1), "off_minus_parent": round(o[len(o) // 2] - p[len(p) // 2], 1),
                                    "unchanged": abs(o[len(o) // 2] - p[len(p) // 2]) <= p[-1] - p[0]}
        if not args.parent_lib:
            del row["parent"]
        res["tokens_per_s"][sampler] = row
    if args.long_ntok:
        row = {}
        for variant in ("off", "dry_last1024", "dry_last4096", "penalties_last1024"):
            row[variant] = tokens("greedy", variant, args.long_ntok)
        over_off(row)
        if not failed:
            row["dry_last1024_minus_penalties_last1024_us"] = round(row["dry_last1024"]["us_per_token_over_off"] - row["penalties_last1024"]["us_per_token_over_off"], 2)
        res["tokens_per_s"]["greedy_n%d" % args.long_ntok] = row
    res["op"] = step("op", ["--child", "op"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
