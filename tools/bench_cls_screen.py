"""What the greedy screen (csrc/cls_screen.h, q4_set_greedy_screen) is worth: bench.py's headline, this build against another build of the library
(--parent-lib: the parent commit's libllama2_q4.so) in ONE session -- boxes differ by +-3 %, so only same-session pairs count.

Each configuration (model, -n) alternates the two libraries, `--rounds` times each; every run is `bench.py --gpus 1 --steps 20 --warmup 5` in a fresh
child process under its own time limit, the library chosen by Q4_LIB_OVERRIDE (a child that fails or runs out of time ends the whole measurement: nothing
more is started on the GPU). Accepted when every run of the change beats every run of the parent and the medians differ by at least twice the parent's own
spread (max - min) in that session. A last child reports the candidate rows per screened step of a 7B -n 256 generation.
Without --parent-lib the switch itself is the A/B (the baseline child calls q4_set_greedy_screen(0), then runs bench.py in the same process).

Writes profiles/cls_screen_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT = [1, 2436, 385, 3686, 388, 1048, 22796, 118]   # bench.py's prompt


def candidates_child(args):
    from llama_cu_awq_amd import api, synth
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    path = os.path.join(args.model_dir, "llama2_q4_synth_7b_seed20240229.bin")
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(synth.GEOMETRIES["7b"])):
        synth.write_model(path, synth.GEOMETRIES["7b"])
    t = api.Transformer(path, temperature=0.0)
    t.generate_ids(PROMPT, 256)
    last, mx, total, steps = t.screen_candidates()
    t.close()
    print("RESULT " + json.dumps({"screened_steps": steps, "mean_candidates": round(total / max(steps, 1), 2), "max_candidates": mx, "vocab": 32000}), flush=True)


def bench_once(args, model, ntok, lib, screen_off):
    env = dict(os.environ)
    if lib:
        env["Q4_LIB_OVERRIDE"] = lib
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--model", model, "--ntok", str(ntok),
           "--model-dir", args.model_dir]
    if screen_off:      # the switch as the A/B: a wrapper child turns it off, then runs bench.py's main in the same process
        cmd = [sys.executable, os.path.abspath(__file__), "--bench-off"] + cmd[2:]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    if p.returncode or not lines:
        raise RuntimeError("bench.py exit status %d: %s" % (p.returncode, p.stderr[-400:]))
    return float(json.loads(lines[-1])["value"])


def median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="7b:256", help="comma-separated model:ntok (the issue's set: 7b:256,13b:256,7b:2048)")
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=400, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_screen_bench.json"))
    ap.add_argument("--candidates-child", action="store_true")
    ap.add_argument("--bench-off", action="store_true")
    args, rest = ap.parse_known_args()
    if args.bench_off:
        import runpy
        from llama_cu_awq_amd import api
        api.lib().q4_set_greedy_screen(0)
        sys.argv = [os.path.join(ROOT, "bench.py")] + rest
        runpy.run_path(sys.argv[0], run_name="__main__")
        return 0
    if args.candidates_child:
        return candidates_child(args)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None
    res = {"command": "bench.py --gpus 1 --steps 20 --warmup 5", "baseline": "the parent commit's library" if parent else "this library, q4_set_greedy_screen(0)", "configs": {}}
    rc = 0
    try:
        for cfg in args.configs.split(","):
            model, ntok = cfg.split(":")
            a, b = [], []
            for r in range(args.rounds):
                a.append(bench_once(args, model, int(ntok), parent, parent is None))
                b.append(bench_once(args, model, int(ntok), None, False))
                print(cfg, "round", r, "baseline %.2f" % a[-1], "screen %.2f" % b[-1], flush=True)
            spread = max(a) - min(a)
            res["configs"][cfg] = {"baseline_tokens_per_s": a, "screen_tokens_per_s": b, "baseline_median": median(a), "screen_median": median(b),
                                   "baseline_spread": round(spread, 2), "gain_percent": round(100.0 * (median(b) / median(a) - 1.0), 2),
                                   "accepted": bool(min(b) > max(a) and median(b) - median(a) >= 2.0 * spread)}
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--candidates-child", "--model-dir", args.model_dir], capture_output=True, text=True,
                           timeout=args.limit, cwd=ROOT)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        res["candidates_7b_256"] = json.loads(lines[-1][7:]) if p.returncode == 0 and lines else {"error": "exit status %d" % p.returncode}
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        res["error"] = str(e)[-600:]
        rc = 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return rc


if __name__ == "__main__":
    sys.exit(main())
