#!/usr/bin/env python3
"""Prompt and verify passes beyond position 256 (q4_set_pass_context; csrc/prompt_pass.hip's split-context attention) measured on the flagship geometry,
7B on one GPU, the bound at its default (256) against the bound at the model's context in the SAME library. Writes profiles/pass_context_bench.json (or
the path given with --out):
  (a) reset to first generated token for prompts of 500 / 1000 / 2000 tokens;
  (b) one prompt pass and one q4_verify_tokens call of n = 2 .. 8 positions at positions 300, 1000 and 2000, against n steps there;
  (c) -n 2048 greedy with the all-accepted and the none-accepted forced drafter at 7 drafts, against speculation off;
  (d) bench.py in three alternating processes each of this build and of another one (--parent-lib: the parent commit's libllama2_q4.so), bound left alone.
Every figure is the median of --reps measurements with [min, max]. Every child process runs under a time limit of its own; one that fails ends the tool.
    tools/bench_pass_context.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5] [--parts abcd]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def open_model(model):
    import ctypes as C
    from llama_cu_awq_amd import api, synth
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    path = os.path.join(os.environ.get("Q4_MODEL_DIR", "/tmp"), "llama2_q4_synth_%s_seed20240229.bin" % model)
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(synth.geometry(model))):
        synth.write_model(path, model)
    return api, L, api.Transformer(path)


def wrong(tok, vocab):
    w = (int(tok) + 1) % vocab
    return w + 1 if w == 2 else w


def measure(model, reps, parts):
    import numpy as np
    api, L, t = open_model(model)
    vocab, S = t.config.vocab_size, t.config.seq_len
    T = L.q4_get_prompt_ingest()
    rng = np.random.default_rng(7)
    text = [1] + [int(x) for x in rng.integers(3, vocab, size=S - 1)]
    res = {"context": S}

    def loop_ms(prompt, steps, start=0):
        """the token loop's own clock over one generation, milliseconds"""
        return 1e3 * t.generate_ids_from(prompt, steps, start)[3]

    # (a) reset to first generated token (the loop's clock stops once the step BEHIND the one it queued last has ended: one more step is queued)
    if "a" in parts:
        res["first_token_ms"] = []
        for n in (500, 1000, 2000):
            row = {"prompt_tokens": n}
            for name, bound in (("bound_256", 256), ("bound_context", S)):
                api.set_pass_context(bound)
                loop_ms(text[:n], n + 1)                      # warm: graphs captured, scratch allocated
                before = L.q4_prompt_passes()
                row[name] = spread([loop_ms(text[:n], n + 1) for _ in range(reps)])
                row[name]["passes_per_run"] = (L.q4_prompt_passes() - before) // reps
            L.q4_set_prompt_ingest(0)
            loop_ms(text[:n], n + 1)
            row["per_token"] = spread([loop_ms(text[:n], n + 1) for _ in range(reps)])
            L.q4_set_prompt_ingest(T)
            row["ratio_256_over_context"] = round(row["bound_256"]["median"] / row["bound_context"]["median"], 3)
            res["first_token_ms"].append(row)
            print("(a)", row, flush=True)

    # (b) one pass at depth. Prompt pass: a run resumed at p over a prompt of p + n + 1 tokens (n prompt-only positions and the generating step) against
    # the same run with a prompt of p + 1 tokens (the generating step alone); the steps' figure is the same difference with prompt ingest off. Verify
    # pass: the host clock around q4_verify_tokens (it synchronises in front and behind) with the run's own continuation as drafts.
    if "b" in parts:
        api.set_pass_context(S)
        res["pass_at_depth"] = {}
        R = t.generate_ids(text[:8], S)[0].copy()             # a greedy run over the whole context: the verify passes' drafts
        assert len(R) == S + 1, "the greedy run ended early"
        for p in (300, 1000, 2000):
            at = {}
            t.generate_ids(text[:p + T + 1], p + T + 2)       # rows [0, p) of `text` in place for the resumed runs below
            base = statistics.median(loop_ms(text[:p + 1], p + 2, p) for _ in range(reps))
            for n in range(2, T + 1):
                prompt = text[:p + n + 1]
                before = L.q4_prompt_passes()
                on = [loop_ms(prompt, p + n + 2, p) - base for _ in range(reps)]
                assert L.q4_prompt_passes() - before == reps, "position %d, %d positions: expected one pass per run" % (p, n)
                L.q4_set_prompt_ingest(0)
                off = [loop_ms(prompt, p + n + 2, p) - base for _ in range(reps)]
                L.q4_set_prompt_ingest(T)
                at[str(n)] = {"prompt_pass_ms": spread(on), "steps_ms": spread(off)}
            t.generate_ids(R[:p + 1], p)                      # the ring and the rows of R up to position p
            for n in range(2, T + 1):
                D = n - 1
                ms = []
                for _ in range(reps + 1):
                    t.generate_ids_from(R[:p + 1], p, p - 1)   # back to position p over the rows in place (an accepted pass wrote R's rows again)
                    assert t.pos() == p
                    api.synchronize()
                    t0 = time.perf_counter()
                    got = t.verify([int(v) for v in R[p + 1:p + 1 + D]])
                    ms.append(1e3 * (time.perf_counter() - t0))
                    assert got is not None and got[1] == D, "the pass is not admitted, or the run's own continuation was not accepted"
                at[str(n)]["verify_pass_ms"] = spread(ms[1:])
                print("(b) position", p, "n", n, at[str(n)], flush=True)
            res["pass_at_depth"][str(p)] = at

    # (c) speculation over a whole context: tokens/s by the loop's clock
    if "c" in parts:
        api.set_pass_context(S)
        R = t.generate_ids(text[:8], S)[0].copy()

        def tokens_per_s():
            t.generate_ids(text[:8], S)
            return [t.generate_ids(text[:8], S)[1] for _ in range(reps)]
        res["speculation"] = {"steps": S, "drafts": 7, "off": spread(tokens_per_s())}
        drafters = {"all_accepted": lambda ring, room: R[len(ring):len(ring) + room],
                    "none_accepted": lambda ring, room: [wrong(R[len(ring)], vocab)] + [int(v) for v in R[len(ring) + 1:len(ring) + room]]}
        t.set_speculative(draft=7, ngram=3, min=1)
        for bound_name, bound, kinds in (("bound_context", S, ("all_accepted", "none_accepted")), ("bound_256", 256, ("all_accepted", "none_accepted"))):
            api.set_pass_context(bound)
            for kind in kinds:
                t.set_drafter(drafters[kind])
                before = t.spec_stats()
                tps = tokens_per_s()
                after = t.spec_stats()
                assert np.array_equal(t.generate_ids(text[:8], S)[0], R), "the speculative run's tokens differ from the run without it"
                res["speculation"]["%s_%s" % (kind, bound_name)] = {"tokens_per_s": spread(tps), "passes_per_run": (after[0] - before[0]) // (reps + 1),
                                                                    "accepted_per_run": (after[2] - before[2]) // (reps + 1)}
                print("(c)", kind, bound_name, res["speculation"]["%s_%s" % (kind, bound_name)], flush=True)
        t.set_drafter(None)
        t.set_speculative(draft=0)
        res["speculation"]["off_again"] = spread(tokens_per_s())
    api.set_pass_context(256)
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_context_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="abcd")
    a = ap.parse_args()
    res = {"model": a.model, "repeats": a.reps}
    if os.path.exists(a.out):          # parts measured by an earlier call stay
        res.update(json.load(open(a.out)))
    if set(a.parts) & set("abc"):
        res.update(measure(a.model, a.reps, a.parts))
    if "d" in a.parts and a.parent_lib:
        res["bench_py_default_bound"] = {"parent": [], "change": []}
        for _ in range(3):
            for who, lib in (("parent", a.parent_lib), ("change", None)):
                env = dict(os.environ)
                if lib:
                    env["Q4_LIB_OVERRIDE"] = lib
                out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--model", a.model],
                                     env=env, capture_output=True, text=True, timeout=300, check=True).stdout
                line = json.loads(out.strip().splitlines()[-1])
                res["bench_py_default_bound"][who].append({"tokens_per_s": line["value"], "per_generation": line.get("tok_s_per_generation")})
                print("(d)", who, line["value"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
