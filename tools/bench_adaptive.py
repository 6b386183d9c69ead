"""What typical-p, top-n-sigma and Mirostat v2 (q4_sampler_set_adaptive, csrc/q4_adaptive.hip) cost, on one MI355X:

  tokens/s and microseconds per token of 7B -n 256 generations -- greedy and the CLI's default sampler (-t 0.5 -p 0.6) -- with everything off,
  top-n-sigma alone, typical-p alone, Mirostat alone and all three behind top-k 40 (a greedy run has no Mirostat: temperature 0 refuses it, so its
  "all three" is top-n-sigma and typical-p behind top-k 40); with --parent-lib (a libllama2_q4.so built from the parent commit) the parent and this
  build's "off" run side by side, `--rounds` (3) interleaved processes each: "unchanged" means the two medians differ by no more than the parent's own
  spread (max - min of its processes), which is recorded.

  the launch alone at n = 32000 (q4_adaptive_mask on the q4 stream, host-timed over back-to-back calls, each with its parameter upload, best of five):
  per stage and all together, on seeded normal logits at scale 3.

Every configuration runs in a fresh child process under its own time limit; a child that fails or runs out of time is reported as such and nothing
more is started. Writes profiles/adaptive_bench.json (or --out)."""
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
SIGMA, TYPICAL, MIROSTAT = dict(top_n_sigma=1.5), dict(typical_p=0.9), dict(mirostat_tau=5.0, mirostat_eta=0.1)
VARIANTS = {                                            # name: (adaptive, sampling)
    "off": (None, None),
    "top_n_sigma": (SIGMA, None),
    "typical_p": (TYPICAL, None),
    "mirostat": (MIROSTAT, None),
    "all_top_k40": (dict(SIGMA, **TYPICAL, **MIROSTAT), dict(top_k=40)),
    "sigma_typical_top_k40": (dict(SIGMA, **TYPICAL), dict(top_k=40)),
}
PER_SAMPLER = {"greedy": ("top_n_sigma", "typical_p", "sigma_typical_top_k40"), "sampled_t0.5_p0.6": ("top_n_sigma", "typical_p", "mirostat", "all_top_k40")}


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
    adaptive, sampling = VARIANTS[args.variant]
    if adaptive is not None:
        t.set_adaptive(**adaptive)
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
    if adaptive is not None:
        import numpy as np
        kept = t.adaptive_records(len(PROMPT) - 1, args.ntok - len(PROMPT))[:, 5].copy().view(np.int32)       # the generating positions
        out["kept_entries_median"] = int(np.median(kept))
    t.close()
    print("RESULT " + json.dumps(out), flush=True)


def child_op(args):
    """microseconds per call over `--op-calls` back-to-back calls and one synchronise, best of five. Top-n-sigma and typical-p are NOT idempotent (a
    second launch takes its statistics over what the first left and truncates further), so every timed call gets a buffer of its own holding the
    fresh logits, refilled outside the timed window."""
    import numpy as np
    api = open_library()
    n = 32000
    x = (np.random.default_rng(1).standard_normal(n) * 3.0).astype(np.float16)
    fresh = np.tile(x, args.op_calls)
    logits = api.DevBuf(fresh)                                 # op_calls copies, 64000 bytes apart (16-byte aligned)
    views = [type("View", (), {"ptr": logits.ptr + 2 * n * i})() for i in range(args.op_calls)]
    mu, side = api.DevBuf(np.full(8, np.nan, dtype=np.float32)), api.DevBuf(nbytes=4 * (n + 2))
    tokens, pos = api.DevBuf(np.zeros(8, dtype=np.int32)), api.DevBuf(np.zeros(1, dtype=np.int32))

    def timed(ctl):
        best = None
        for batch in range(6):                                 # (the first batch warms up)
            logits.put(fresh)
            mu.put(np.full(8, np.nan, dtype=np.float32))       # position 0: a span starts in every call
            api.synchronize()
            t0 = time.perf_counter()
            for v in views:
                api.adaptive_mask(v, n, temperature=0.8, mu_ring=mu, side=side, tokens=tokens, pos=pos, **ctl)
            api.synchronize()
            dt = (time.perf_counter() - t0) / args.op_calls * 1e6
            if batch:
                best = dt if best is None else min(best, dt)
        return round(best, 2)

    out = {"calls": args.op_calls, "vocabulary": n,
           "note": "every timed call runs on its own copy of the fresh logits (refilled outside the timed window); host clock around op-calls "
                   "back-to-back launches and one synchronise, each launch with its 32-byte parameter upload in stream order"}
    for name, ctl in (("top_n_sigma", SIGMA), ("typical_p", TYPICAL), ("mirostat", MIROSTAT), ("all", dict(SIGMA, **TYPICAL, **MIROSTAT))):
        out[name] = {"us_per_call": timed(ctl)}
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved processes of the parent and of this build's off")
    ap.add_argument("--op-calls", type=int, default=1000)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=400, help="seconds per child (the first one writes the model file)")
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit, run side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_bench.json"))
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
                   "back-to-back calls, each with its parameter upload"}
    failed = False

    def step(name, argv, **kw):
        nonlocal failed
        if failed:               # (a child that failed on the GPU: start nothing more there)
            return {"error": "not started"}
        r = run_child(args, argv, **kw)
        print(name, r, flush=True)
        failed = "error" in r
        return r

    def tokens(sampler, variant, lib=None):
        return step("%s %s%s" % (sampler, variant, " (parent)" if lib else ""),
                    ["--child", "tokens", "--sampler", sampler, "--variant", variant, "--ntok", str(args.ntok)], lib=lib)

    for sampler in SAMPLERS:
        row = {"off": [], "parent": []}
        for _ in range(args.rounds):
            if args.parent_lib:
                row["parent"].append(tokens(sampler, "off", lib=args.parent_lib))
            row["off"].append(tokens(sampler, "off"))
        for variant in PER_SAMPLER[sampler]:
            row[variant] = tokens(sampler, variant)
        offs = [r["tokens_per_s_best"] for r in row["off"] if "tokens_per_s_best" in r]
        for name, r in row.items():
            if offs and isinstance(r, dict) and "tokens_per_s_best" in r:
                r["us_per_token"] = round(1e6 / r["tokens_per_s_best"], 2)
                r["us_per_token_over_off"] = round(1e6 / r["tokens_per_s_best"] - 1e6 / max(offs), 2)
        if args.parent_lib and not failed:
            med = lambda rs: sorted(r["tokens_per_s_median"] for r in rs)
            p, o = med(row["parent"]), med(row["off"])
            row["off_vs_parent"] = {"parent_median": p[len(p) // 2], "parent_spread": round(p[-1] - p[0], 1), "off_median": o[len(o) // 2],
                                    "off_spread": round(o[-1] - o[0], 1), "off_minus_parent": round(o[len(o) // 2] - p[len(p) // 2], 1),
                                    "unchanged": abs(o[len(o) // 2] - p[len(p) // 2]) <= p[-1] - p[0]}
        if not args.parent_lib:
            del row["parent"]
        res["tokens_per_s"][sampler] = row
    res["op"] = step("op", ["--child", "op"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
