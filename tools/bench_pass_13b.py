#!/usr/bin/env python3
"""Prompt and verify passes for the Llama-2-13B shape (q4_set_pass_13b; DESIGN.md 3.7 "13B") measured on the `13b`
synthetic checkpoint (dim 5120, hidden 13824, 40 layers, 40 heads, vocabulary 32000, context 2048). Writes
profiles/pass_13b_bench.json (or the path given with --out):
  (a) ingest: reset to first generated token, the switch off against on in the same library, for 8 / 64 / 250 prompt tokens and -- with
      q4_set_pass_context(2048) -- 500 / 1000 / 2000;
  (b) one pass against steps: positions p .. p + n - 1 as ONE prompt pass (switch on) against n per-token prompt steps (switch off), n = 2 .. 8 at
      p = 30, 300 and 2000, through the same entry (q4_generate_ids_from over rows [0, p) in place), host clock around a call that synchronises --
      the shipped library admits passes of this shape from four positions on (prompt_pass_min), so n = 2 and 3 are passes only in a build with
      make exp EXPFLAGS=-DQ4_PP13_MIN=2 given as Q4_LIB_OVERRIDE (the figures that set the minimum were taken so); else they are marked not admitted;
  (c) speculation: -n 256 greedy -- off; 1, 3 and 7 drafts per pass with every draft accepted; 7 drafts with none accepted -- and the break-even
      number of accepted drafts per pass;
  (d) nothing changed with the switch off: bench.py --gpus 1 --steps 20 --warmup 5 on 7b and on 13b against another build of the library
      (--parent-lib: the parent commit's libllama2_q4.so), three processes of each, alternating.
  (e) --variant-libs NAME=PATH ...: experiment builds of the library (make exp EXPFLAGS=-DQ4_PP_FFN13_WAVES=12: gate / up in twelve-wave blocks) beside this
      one, a process each, alternating three times: reset to first generated token for 64 and 250 prompt tokens with the switch on.
Medians of --reps with [min, max]. The weights are synthetic.
    tools/bench_pass_13b.py [--out FILE] [--parent-lib PATH] [--variant-libs NAME=PATH ...] [--model 13b] [--reps 5] [--skip abcd]"""
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


def measure(model, reps, skip, res, save):
    import numpy as np
    api, L = open_library()
    t = api.Transformer(model_path(model))
    vocab, seq_len = t.config.vocab_size, t.config.seq_len
    rng = np.random.default_rng(7)
    long_prompt = [1] + [int(x) for x in rng.integers(3, vocab, size=seq_len - 1)]

    def first_token_ms(prompt):
        steps = len(prompt) + 1      # the loop's clock stops once the step BEHIND the one it queued last has ended: queue one more
        t.generate_ids(prompt, steps)
        return [1e3 * t.generate_ids(prompt, steps)[3] for _ in range(reps)]

    if "a" not in skip:
        res["first_token_ms"] = []
        for n, bound in ((8, 256), (64, 256), (250, 256), (500, 2048), (1000, 2048), (2000, 2048)):
            api.set_pass_context(bound)
            prompt = long_prompt[:n]
            row = {"prompt_tokens": n, "pass_context": bound}
            t.set_pass_13b(False)
            before = api.prompt_passes()
            row["switch_off"] = spread(first_token_ms(prompt))
            assert api.prompt_passes() == before
            t.set_pass_13b(True)
            before = api.prompt_passes()
            row["switch_on"] = spread(first_token_ms(prompt))
            row["passes"] = (api.prompt_passes() - before) // (reps + 1)
            row["ratio"] = round(row["switch_off"]["median"] / row["switch_on"]["median"], 3)
            res["first_token_ms"].append(row)
            print("first token", row, flush=True)
        api.set_pass_context(256)
        save()

    if "b" not in skip:
        api.set_pass_context(seq_len)
        res["pass_against_steps_ms"] = []
        for p in (30, 300, 2000):
            t.set_pass_13b(True)
            t.generate_ids(long_prompt[:p + 1], p)
            for n in range(2, 9):
                row = {"position": p, "n": n}
                prompt = long_prompt[:p + n + 1]
                for on in (False, True):
                    t.set_pass_13b(on)
                    ms = []
                    before = api.prompt_passes()
                    for _ in range(reps + 1):
                        api.synchronize()
                        t0 = time.perf_counter()
                        t.generate_ids_from(prompt, p + n, p)
                        api.synchronize()
                        ms.append(1e3 * (time.perf_counter() - t0))
                    ran = api.prompt_passes() - before
                    assert ran == 0 if not on else ran in (0, reps + 1), (p, n, on, ran)
                    if on and ran == 0:       # below the shape's admitted minimum (prompt_pass_min): the shipped library runs steps here
                        row["pass_admitted"] = False
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
        t.set_pass_13b(False)
        off = tokens_per_s()
        R = t.generate_ids(PROMPT_IDS, STEPS)[0].copy()
        spec = {"no_speculation_tokens_per_s": spread(off)}
        step_ms = 1e3 / statistics.median(off)
        t.set_pass_13b(True)
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


def child_variant(model, reps):
    """one process: reset to first generated token with the switch on, ms"""
    import numpy as np
    api, _ = open_library()
    t = api.Transformer(model_path(model), pass_13b=True)
    rng = np.random.default_rng(7)
    out = {}
    for n in (64, 250):
        prompt = [1] + [int(x) for x in rng.integers(3, t.config.vocab_size, size=n - 1)]
        t.generate_ids(prompt, n + 1)
        out[str(n)] = [1e3 * t.generate_ids(prompt, n + 1)[3] for _ in range(reps)]
    print(json.dumps(out))
    t.close()


def bench_py(model, lib):
    env = dict(os.environ)
    if lib:
        env["Q4_LIB_OVERRIDE"] = lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--model", model], env=env,
                         capture_output=True, text=True, timeout=900, check=True).stdout
    r = json.loads(out.strip().splitlines()[-1])
    return spread(r["tok_s_per_generation"]) if r.get("tok_s_per_generation") else {"median": r["value"], "min": r["value"], "max": r["value"], "n": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_13b_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="13b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="", help="letters of the sections to leave out")
    ap.add_argument("--variant-libs", nargs="*", default=[], metavar="NAME=PATH")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child_variant(a.model, a.reps)
    res = {"model": a.model, "steps": STEPS, "repeats": a.reps}
    if os.path.exists(a.out):           # sections measured by an earlier call stay
        res.update(json.load(open(a.out)))

    def save():                         # after every section: a call that runs out of time keeps what it measured
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    if a.parent_lib and "d" not in a.skip:
        res["off_against_parent"] = {}
        for model in ("7b", a.model):
            row = {"parent": [], "change": []}
            for _ in range(3):
                for who, lib in (("parent", a.parent_lib), ("change", None)):
                    row[who].append(bench_py(model, lib))
                    print(model, who, row[who][-1], flush=True)
            p = [r["median"] for r in row["parent"]]
            c = [r["median"] for r in row["change"]]
            row["parent_medians_min_max"] = [min(p), max(p)]
            row["change_medians_min_max"] = [min(c), max(c)]
            row["change_minus_parent_medians"] = round(statistics.median(c) - statistics.median(p), 3)
            row["change_inside_parent_spread"] = bool(min(p) <= statistics.median(c) <= max(p))
            res["off_against_parent"][model] = row
            save()
    if a.variant_libs:
        libs = [("shipped", None)] + [tuple(v.split("=", 1)) for v in a.variant_libs]
        rows = {name: {"64": [], "250": []} for name, _ in libs}
        for _ in range(3):
            for name, lib in libs:
                env = dict(os.environ)
                if lib:
                    env["Q4_LIB_OVERRIDE"] = os.path.abspath(lib)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "variant", "--model", a.model, "--reps", str(a.reps)], env=env,
                                     capture_output=True, text=True, timeout=600, check=True).stdout
                got = json.loads(out.strip().splitlines()[-1])
                for n in rows[name]:
                    rows[name][n] += got[n]
                print("variant", name, {n: spread(v) for n, v in got.items()}, flush=True)
        res["variants_first_token_ms"] = {name: {n: spread(v) for n, v in r.items()} for name, r in rows.items()}
        save()
    measure(a.model, a.reps, a.skip, res, save)
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
