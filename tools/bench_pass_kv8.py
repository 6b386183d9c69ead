#!/usr/bin/env python3
"""Prompt and verify passes on the FP8 (e4m3) K / V cache (q4_set_pass_kv8; DESIGN.md 3.7 "FP8 cache") measured on the synthetic 7B checkpoint built
with kv="fp8" (dim 4096, hidden 11008, 32 layers, vocabulary 32000). Writes profiles/pass_kv8_bench.json (or the path given with --out):
  (a) ingest: reset to first generated token, the switch off against on in the same library, for 8 / 64 / 250 prompt tokens, with
      q4_set_pass_context(2048) 500 / 1000 / 2000 and, on `7b_16k` with the bound at 16384, 4000 / 8000 (--long-model; --skip l leaves it out);
  (b) one pass against steps: positions p .. p + n - 1 as ONE prompt pass (switch on) against n per-token prompt steps (switch off), n = 2 .. 8 at
      p = 30, 300 and 2000, through the same entry (q4_generate_ids_from over rows [0, p) in place), host clock around a call that synchronises;
      and the append launch's share of a pass, from a kernel trace of the 250-token ingest (--kernel-stats FILE: the kernel statistics CSV that
      `rocprofv3 --kernel-trace --stats -- tools/bench_pass_kv8.py --child fp8,passes` writes): its time over that of all the pass's launches;
  (c) speculation: -n 256 greedy -- off; 1, 3 and 7 drafts per pass with every draft accepted; 7 drafts with none accepted -- and the break-even
      number of accepted drafts per pass;
  (d) nothing changed with the switch off (--parent-lib: the parent commit's libllama2_q4.so), three processes of each build, alternating:
      bench.py --gpus 1 --steps 20 --warmup 5 on 7b (fp16 cache); the same loop (bench.py's prompt, -n 256, 5 warm-up and 20 timed generations) on 7b
      with kv="fp8" in a child of this tool (bench.py builds its model with the fp16 cache); and the fp16 250-token ingest.
Medians of --reps with [min, max]. The weights are synthetic.
    tools/bench_pass_kv8.py [--out FILE] [--parent-lib PATH] [--model 7b] [--long-model 7b_16k] [--reps 5] [--skip abcdl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT_IDS = [1, 2436, 385, 3686, 388, 1048, 22796, 118]   # bench.py's
STEPS = 256


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def model_path(model):
    from llama_cu_awq_amd import synth
    path = os.path.join(os.environ.get("Q4_MODEL_DIR", "/tmp"), "llama2_q4_synth_%s_seed20240229.bin" % model)
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(synth.geometry(model))):
        synth.write_model(path, model)
    return path


def open_library():
    from llama_cu_awq_amd import api
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    return api, L


def wrong(tok, vocab):
    w = (int(tok) + 1) % vocab
    return w + 1 if w == 2 else w


def long_prompt_of(t):
    import numpy as np
    rng = np.random.default_rng(7)
    return [1] + [int(x) for x in rng.integers(3, t.config.vocab_size, size=t.config.seq_len - 1)]


def first_token_rows(api, t, cases, reps):
    prompt_all = long_prompt_of(t)

    def first_token_ms(prompt):
        steps = len(prompt) + 1      # the loop's clock stops once the step BEHIND the one it queued last has ended: queue one more
        t.generate_ids(prompt, steps)
        return [1e3 * t.generate_ids(prompt, steps)[3] for _ in range(reps)]
    rows = []
    for n, bound in cases:
        api.set_pass_context(bound)
        prompt = prompt_all[:n]
        row = {"prompt_tokens": n, "pass_context": bound}
        t.set_pass_kv8(False)
        before = api.prompt_passes()
        row["switch_off"] = spread(first_token_ms(prompt))
        assert api.prompt_passes() == before
        t.set_pass_kv8(True)
        before = api.prompt_passes()
        row["switch_on"] = spread(first_token_ms(prompt))
        row["passes"] = (api.prompt_passes() - before) // (reps + 1)
        row["ratio"] = round(row["switch_off"]["median"] / row["switch_on"]["median"], 3)
        row["pass_wins"] = bool(row["switch_on"]["median"] < row["switch_off"]["median"])
        rows.append(row)
        print("first token", row, flush=True)
    api.set_pass_context(256)
    return rows


def measure(model, long_model, reps, skip, res, save):
    import numpy as np
    api, L = open_library()
    t = api.Transformer(model_path(model), kv="fp8")
    vocab, seq_len = t.config.vocab_size, t.config.seq_len
    long_prompt = long_prompt_of(t)

    if "a" not in skip:
        res["first_token_ms"] = first_token_rows(api, t, ((8, 256), (64, 256), (250, 256), (500, 2048), (1000, 2048), (2000, 2048)), reps)
        save()

    if "b" not in skip:
        api.set_pass_context(seq_len)
        res["pass_against_steps_ms"] = []
        for p in (30, 300, 2000):
            t.set_pass_kv8(True)
            t.generate_ids(long_prompt[:p + 1], p)
            for n in range(2, 9):
                row = {"position": p, "n": n}
                prompt = long_prompt[:p + n + 1]
                for on in (False, True):
                    t.set_pass_kv8(on)
                    ms = []
                    before = api.prompt_passes()
                    for _ in range(reps + 1):
                        api.synchronize()
                        t0 = time.perf_counter()
                        t.generate_ids_from(prompt, p + n, p)
                        api.synchronize()
                        ms.append(1e3 * (time.perf_counter() - t0))
                    assert api.prompt_passes() - before == ((reps + 1) if on else 0), (p, n, on)
                    row["pass" if on else "steps"] = spread(ms[1:])
                row["ratio"] = round(row["steps"]["median"] / row["pass"]["median"], 3)
                row["pass_wins"] = bool(row["pass"]["median"] < row["steps"]["median"])
                res["pass_against_steps_ms"].append(row)
                print("pass against steps", row, flush=True)
        api.set_pass_context(256)
        save()

    if "c" not in skip:
        def tokens_per_s():
            return [t.generate_ids(PROMPT_IDS, STEPS)[1] for _ in range(reps + 1)][1:]
        t.set_pass_kv8(False)
        off = tokens_per_s()
        R = t.generate_ids(PROMPT_IDS, STEPS)[0].copy()
        spec = {"no_speculation_tokens_per_s": spread(off)}
        step_ms = 1e3 / statistics.median(off)
        t.set_pass_kv8(True)
        cases = [("all_accepted_draft_%d" % d, d, lambda ring, room: R[len(ring):len(ring) + room]) for d in (1, 3, 7)]
        cases.append(("none_accepted_draft_7", 7, lambda ring, room: [wrong(R[len(ring)], vocab)] + [int(v) for v in R[len(ring) + 1:len(ring) + room]]))
        for kind, draft, fn in cases:
            t.set_speculative(draft=draft, ngram=3, min=1)
            t.set_drafter(fn)
            before = t.spec_stats()
            tps = tokens_per_s()
            after = t.spec_stats()
            same = bool(np.array_equal(t.generate_ids(PROMPT_IDS, STEPS)[0], R))
            spec[kind] = {"tokens_per_s": spread(tps), "passes_per_run": (after[0] - before[0]) // (reps + 1), "accepted_per_run": (after[2] - before[2]) // (reps + 1),
                          "ratio_to_no_speculation": round(statistics.median(tps) / statistics.median(off), 3), "same_tokens": same}
            print("speculation", kind, spec[kind], flush=True)
        # a pass of eight rows that accepts nothing yields one token in pass_ms; it pays from the a accepted drafts at which (1 + a) * step_ms > pass_ms
        pass_ms = 1e3 / spec["none_accepted_draft_7"]["tokens_per_s"]["median"]
        spec["step_ms"], spec["pass_of_8_ms"] = round(step_ms, 4), round(pass_ms, 4)
        spec["break_even_accepted_drafts_per_pass"] = round(pass_ms / step_ms - 1.0, 3)
        t.set_drafter(None)
        t.set_speculative(draft=0)
        res["speculation_n256_greedy"] = spec
        save()
    t.close()

    if "l" not in skip:      # the long context: the case the switch exists for
        t = api.Transformer(model_path(long_model), kv="fp8")
        res["first_token_ms_long"] = {"model": long_model, "rows": first_token_rows(api, t, ((4000, 16384), (8000, 16384)), max(2, reps // 2))}
        t.close()
        save()


def child_off(model, kv, what):
    """one process, the switch off: bench.py's loop with the given cache format (tokens/s per generation), or the 250-token ingest (ms)"""
    api, _ = open_library()
    t = api.Transformer(model_path(model), kv=kv)
    if what == "passes":     # (for a kernel trace) five 250-token ingests by passes
        t.set_pass_kv8(True)
        prompt = long_prompt_of(t)[:250]
        for _ in range(5):
            t.generate_ids(prompt, 251)
        print(json.dumps([0.0]))
    elif what == "decode":
        for _ in range(5):
            t.generate_ids(PROMPT_IDS, STEPS)
        out = [t.generate_ids(PROMPT_IDS, STEPS)[1] for _ in range(20)]
    else:
        prompt = long_prompt_of(t)[:250]
        t.generate_ids(prompt, 251)
        out = [1e3 * t.generate_ids(prompt, 251)[3] for _ in range(10)]
    print(json.dumps(out))
    t.close()


def run_child(model, kv, what, lib):
    env = dict(os.environ)
    if lib:
        env["Q4_LIB_OVERRIDE"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s,%s" % (kv, what), "--model", model], env=env, capture_output=True, text=True,
                         timeout=900, check=True).stdout
    return spread(json.loads(out.strip().splitlines()[-1]))


def bench_py(model, lib):
    env = dict(os.environ)
    if lib:
        env["Q4_LIB_OVERRIDE"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--model", model], env=env,
                         capture_output=True, text=True, timeout=900, check=True).stdout
    r = json.loads(out.strip().splitlines()[-1])
    return spread(r["tok_s_per_generation"]) if r.get("tok_s_per_generation") else {"median": r["value"], "min": r["value"], "max": r["value"], "n": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_kv8_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--long-model", default="7b_16k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="", help="letters of the sections to leave out (l: the long-context ingest)")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        kv, what = a.child.split(",")
        return child_off(a.model, kv, what)
    res = {"model": a.model, "kv": "fp8", "steps": STEPS, "repeats": a.reps}
    if os.path.exists(a.out):           # sections measured by an earlier call stay
        res.update(json.load(open(a.out)))

    def save():                         # after every section: a call that runs out of time keeps what it measured
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    if a.kernel_stats:
        import csv
        tot, app = 0.0, 0.0
        for r in csv.DictReader(open(a.kernel_stats)):
            name, ns = r.get("Name", ""), float(r.get("TotalDurationNs", 0) or 0)
            if "prompt_" in name or "pass_kv8" in name or ("attention_kv8_kernel" in name and "true>" in name):     # (the row form of the one-pass kernel)
                tot += ns
                app += ns if "pass_kv8_append" in name else 0.0
        res["append_share_of_pass_launches"] = {"prompt_tokens": 250, "append_ns": app, "pass_launches_ns": tot, "share": round(app / tot, 5) if tot else None}
        save()
        print("append share", res["append_share_of_pass_launches"])
        return
    if a.parent_lib and "d" not in a.skip:
        res["off_against_parent"] = {}
        legs = (("7b_fp16_bench_py_tokens_per_s", lambda lib: bench_py(a.model, lib), True),
                ("7b_fp8_decode_tokens_per_s", lambda lib: run_child(a.model, "fp8", "decode", lib), True),
                ("7b_fp16_ingest_250_ms", lambda lib: run_child(a.model, "fp16", "ingest", lib), False))
        for name, leg, _ in legs:
            row = {"parent": [], "change": []}
            for _ in range(3):
                for who, lib in (("parent", a.parent_lib), ("change", None)):
                    row[who].append(leg(lib))
                    print(name, who, row[who][-1], flush=True)
            p = [r["median"] for r in row["parent"]]
            c = [r["median"] for r in row["change"]]
            row["parent_medians_min_max"] = [min(p), max(p)]
            row["change_medians_min_max"] = [min(c), max(c)]
            row["change_minus_parent_medians"] = round(statistics.median(c) - statistics.median(p), 3)
            row["change_inside_parent_spread"] = bool(min(p) <= statistics.median(c) <= max(p))
            res["off_against_parent"][name] = row
            save()
    measure(a.model, a.long_model, a.reps, a.skip, res, save)
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
