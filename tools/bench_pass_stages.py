#!/usr/bin/env python3
"""Logit stages inside verify passes and the guide's forced drafts (q4_set_pass_stages; DESIGN.md 3.8 "Under the logit stages") measured on the 7B
synthetic checkpoint at -n 256. Writes profiles/pass_stages_bench.json (or the path given with --out):
  (a) the switch off against another build of the library (--parent-lib: the parent commit's libllama2_q4.so): three fresh processes of each,
      alternating, greedy and -t 0.5 -p 0.6;
  (b) one verify pass of n = 2 .. 8 rows with each stage's row launch and with all three, against the same pass without, in one process;
  (c) forced drafts: a from_choices guide of 16 choices x 24 tokens, guided steps against guided steps with forced drafts; tokens/s and accepted
      drafts per pass;
  (d) a drafter that returns the run's own continuation and one that is always wrong, under top-k 40 + repeat penalty 1.1 and under DRY;
  (e) prompt ingest under a guide: reset to first generated token for 64 and 250 prompt tokens, the switch off and on.
Every tokens/s figure is the token loop's own (timed tokens over its seconds, the clock bench.py reads), median of --reps generations with [min, max].
    tools/bench_pass_stages.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5] [--skip abcde]"""
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
SAMPLED = dict(temperature=0.5, topp=0.6, seed=2024)
CONTROLS = dict(top_k=40, repeat_penalty=1.1, penalty_last_n=64)
DRY = dict(multiplier=0.8, no_repeat_ngram_size=4)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def open_lib():
    from llama_cu_awq_amd import api
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    return api, L


def model_path(model):
    from llama_cu_awq_amd import synth
    path = os.path.join(os.environ.get("Q4_MODEL_DIR", "/tmp"), "llama2_q4_synth_%s_seed20240229.bin" % model)
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(synth.geometry(model))):
        synth.write_model(path, model)
    return path


def vocab_of(model):
    from llama_cu_awq_amd import synth
    return synth.geometry(model)[5]


def tokens_per_s(t, reps, prompt=PROMPT_IDS, steps=STEPS):
    t.generate_ids(prompt, steps)                               # warm: graphs captured, scratch allocated
    return [t.generate_ids(prompt, steps)[1] for _ in range(reps)]


def child_off(model, reps, sampled):
    """one process: the switch off (a build without the feature has nothing to switch), tokens/s of `reps` generations"""
    api, _ = open_lib()
    t = api.Transformer(model_path(model), **(SAMPLED if sampled else {}))
    print(json.dumps({"tokens_per_s": tokens_per_s(t, reps)}))
    t.close()


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def sampler_struct(handle):
    return C.cast(handle, C.POINTER(SamplerStruct)).contents


def wrong(tok, vocab):
    w = (int(tok) + 1) % vocab
    return w + 1 if w == 2 else w


def stage_rows_cost(api, model, reps):
    """(b) q4_verify_tokens_sampled at position 20 by the host clock (it synchronises in front and behind), the run's own continuation as drafts"""
    import numpy as np
    res = {}
    for name, kw in (("none", {}), ("guide", "guide"), ("dry", dict(dry=DRY)), ("controls", dict(sampling=CONTROLS)), ("all", "all")):
        g = None
        if kw in ("guide", "all"):
            rng = np.random.default_rng(3)
            table = np.full((64, vocab_of(model)), 0xFFFF, dtype=np.uint16)
            on = rng.random(table.shape) < 0.3
            on[:, 2] = False
            on[np.arange(64), rng.integers(3, table.shape[1], 64)] = True
            table[on] = rng.integers(0, 64, int(on.sum())).astype(np.uint16)
            g = api.Guide(table)
            kw = dict(guide=g) if kw == "guide" else dict(guide=g, dry=DRY, sampling=CONTROLS)
        t = api.Transformer(model_path(model), pass_stages=True, **dict(SAMPLED, **kw))
        t.set_speculative(draft=0, sampled=True)
        R = t.generate_ids(PROMPT_IDS, 40)[0].copy()
        row = {}
        for n in range(2, 9):
            ms = []
            for _ in range(reps + 1):
                api.check(api.lib().q4_set_speculative(t.h, 0, 0, 0))
                sampler_struct(t.sampler).rng_state = SAMPLED["seed"]   # the stream that gave R: it stands at position 20's coin behind these steps
                t.generate_ids(PROMPT_IDS, 20)
                api.synchronize()
                t0 = time.perf_counter()
                got = t.verify_sampled([int(v) for v in R[21:20 + n]])
                ms.append(1e3 * (time.perf_counter() - t0))
                assert got is not None and got[1] == n - 1, "the pass is not admitted, or the run's own continuation was not accepted"
            row[str(n)] = spread(ms[1:])
        res[name] = row
        print("(b)", name, row, flush=True)
        t.close()
        if g is not None:
            g.close()
    return res


def forced(api, model, reps):
    """(c) 16 choices x 24 tokens behind a shared first token; every run ends at the EOS with no step to spare"""
    import numpy as np
    from llama_cu_awq_amd import guide
    vocab = vocab_of(model)
    r = np.random.default_rng(3)
    first = int(r.integers(3, vocab))
    seconds = r.choice(np.arange(3, vocab), size=16, replace=False)
    seqs = [[first, int(s)] + [int(x) for x in r.integers(3, vocab, size=22)] for s in seconds]
    g = api.Guide(guide.from_choices(seqs, vocab))
    steps = len(PROMPT_IDS) + 25
    res = {}
    for name, on in (("guided_steps", False), ("guided_forced_drafts", True)):
        t = api.Transformer(model_path(model), guide=g, pass_stages=on)
        if on:
            t.set_speculative(draft=7, ngram=3, min=1)
        before = t.spec_stats()
        tps = tokens_per_s(t, reps, steps=steps)
        after = t.spec_stats()
        passes = after[0] - before[0]
        res[name] = {"tokens_per_s": spread(tps), "passes_per_run": passes // (reps + 1), "accepted_per_pass": round((after[2] - before[2]) / passes, 3) if passes else 0.0,
                     "forced": t.spec_stats_forced() if on else None}
        print("(c)", name, res[name], flush=True)
        t.close()
    res["speedup"] = round(res["guided_forced_drafts"]["tokens_per_s"]["median"] / res["guided_steps"]["tokens_per_s"]["median"], 3)
    g.close()
    return res


def drafters(api, model, reps):
    """(d) section 3.8's table (c) with stages on"""
    import numpy as np
    res = {}
    for name, kw in (("top_k40_repeat1.1", dict(sampling=CONTROLS)), ("dry", dict(dry=DRY))):
        t = api.Transformer(model_path(model), pass_stages=True, **kw)
        vocab = t.config.vocab_size
        off = tokens_per_s(t, reps)
        R = t.generate_ids(PROMPT_IDS, STEPS)[0].copy()
        row = {"steps": spread(off)}
        t.set_speculative(draft=7, ngram=3, min=1)
        for kind, fn in (("all_accepted", lambda ring, room: R[len(ring):len(ring) + room]),
                         ("none_accepted", lambda ring, room: [wrong(R[len(ring)], vocab)] + [int(v) for v in R[len(ring) + 1:len(ring) + room]])):
            t.set_drafter(fn)
            before = t.spec_stats()
            tps = tokens_per_s(t, reps)
            after = t.spec_stats()
            assert np.array_equal(t.generate_ids(PROMPT_IDS, STEPS)[0], R), "the speculative run's tokens differ from the run without it"
            row[kind] = {"tokens_per_s": spread(tps), "passes_per_run": (after[0] - before[0]) // (reps + 1), "accepted_per_run": (after[2] - before[2]) // (reps + 1)}
        row["speedup_all_accepted"] = round(row["all_accepted"]["tokens_per_s"]["median"] / statistics.median(off), 3)
        res[name] = row
        print("(d)", name, row, flush=True)
        t.close()
    return res


def ingest(api, model, reps):
    """(e) q4_reset_sequence to the first generated token, by the host clock, with a guide attached"""
    import numpy as np
    vocab = vocab_of(model)
    table = np.zeros((4, vocab), dtype=np.uint16)
    table[:, :3] = 0xFFFF
    g = api.Guide(table)
    res = {}
    for n in (64, 250):
        prompt = [1] + [int(x) for x in np.random.default_rng(n).integers(3, vocab, size=n - 1)]
        for name, on in (("off", False), ("on", True)):
            t = api.Transformer(model_path(model), guide=g, pass_stages=on)
            ms = []
            for _ in range(reps + 1):
                api.synchronize()
                t0 = time.perf_counter()
                t.generate_ids(prompt, n)
                ms.append(1e3 * (time.perf_counter() - t0))
            res["%d_%s" % (n, name)] = spread(ms[1:])
            print("(e)", n, name, res["%d_%s" % (n, name)], flush=True)
            t.close()
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_stages_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child in ("off", "off_sampled"):
        return child_off(a.model, a.reps, a.child == "off_sampled")
    res = {"model": a.model, "steps": STEPS, "repeats": a.reps}
    if a.parent_lib and "a" not in a.skip:
        res["off_against_parent"] = {}
        for mode in ("off", "off_sampled"):
            rows = {"parent": [], "change": []}
            for _ in range(3):
                for who, lib in (("parent", a.parent_lib), ("change", None)):
                    env = dict(os.environ)
                    if lib:
                        env["Q4_LIB_OVERRIDE"] = lib
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--model", a.model, "--reps", str(a.reps)], env=env,
                                         capture_output=True, text=True, timeout=600, check=True).stdout
                    rows[who].append(spread(json.loads(out.strip().splitlines()[-1])["tokens_per_s"]))
                    print("(a)", mode, who, rows[who][-1], flush=True)
            res["off_against_parent"]["greedy" if mode == "off" else "t0.5_p0.6"] = rows
    api, _ = open_lib()
    for key, name, fn in (("b", "stage_rows_pass_ms", stage_rows_cost), ("c", "forced_drafts", forced), ("d", "drafters", drafters), ("e", "prompt_ingest_ms", ingest)):
        if key not in a.skip:
            res[name] = fn(api, a.model, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
