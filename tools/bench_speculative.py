#!/usr/bin/env python3
"""Speculative greedy decoding (csrc/spec_verify.h, q4_set_speculative) measured on the flagship workload: 7B, -n 256, greedy, the benchmark's prompt.
Writes profiles/speculative_bench.json (or the path given with --out):
  (a) speculation off against another build of the library (--parent-lib: the parent commit's libllama2_q4.so): three processes of each, alternating;
  (b) one verify pass of n = 2 .. 8 positions, and the classifier and accept launches alone;
  (c) the bounds: a drafter that returns the run's own continuation (every draft accepted) and one whose first token is wrong (none), at 1, 3, 7 drafts,
      and from them the acceptance at which a pass breaks even;
  (d) the built-in prompt-lookup drafter on the same prompt, with its counters.
Every tokens/s figure is the token loop's own (timed tokens over its seconds, the clock bench.py reads), median of --reps generations with min and max.
    tools/bench_speculative.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5]"""
import argparse
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
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


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


def tokens_per_s(t, reps):
    t.generate_ids(PROMPT_IDS, STEPS)                           # warm: graphs captured, scratch allocated
    return [t.generate_ids(PROMPT_IDS, STEPS)[1] for _ in range(reps)]


def child_off(model, reps):
    """one process: speculation off (a build without the feature has nothing to switch), tokens/s of `reps` generations"""
    _, _, t = open_model(model)
    print(json.dumps({"tokens_per_s": tokens_per_s(t, reps)}))
    t.close()


def wrong(tok, vocab):
    w = (int(tok) + 1) % vocab
    return w + 1 if w == 2 else w


def measure(model, reps):
    import ctypes as C
    import numpy as np
    api, L, t = open_model(model)
    vocab, dim = t.config.vocab_size, t.config.dim
    res = {}
    off = tokens_per_s(t, reps)
    R = t.generate_ids(PROMPT_IDS, STEPS)[0].copy()
    res["off_tokens_per_s"] = spread(off)
    step_ms = 1e3 / statistics.median(off)

    # (b) one pass at position 20, by the host clock around q4_verify_tokens (it synchronises in front and behind); the two new launches alone on the
    # model's own wcls, twenty back to back between two synchronisations
    res["pass_ms_by_positions"] = {}
    w = t.weights.contents
    x = api.DevBuf(np.random.default_rng(1).standard_normal((8, dim)).astype(np.float16))
    rows = api.DevBuf(nbytes=8 * vocab * 2)
    lo, xo = api.DevBuf(nbytes=vocab * 2), api.DevBuf(nbytes=dim * 2)
    ring, ph, pd = api.DevBuf(nbytes=64 * 4), api.DevBuf(nbytes=16), api.DevBuf(nbytes=16)

    def launches_ms(fn, k=20):
        fn()
        api.synchronize()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            api.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / k)
        return out

    for n in range(2, 9):
        D = n - 1
        ms = []
        for _ in range(reps + 1):
            t.generate_ids(PROMPT_IDS, 20)
            api.synchronize()
            t0 = time.perf_counter()
            got = t.verify([int(v) for v in R[21:21 + D]])
            ms.append(1e3 * (time.perf_counter() - t0))
            assert got is not None and got[1] == D, "the pass is not admitted, or the run's own continuation was not accepted"
        cls = launches_ms(lambda: api.check(L.q4_verify_classifier(rows.ptr, x.ptr, w.rms_final_weight, w.wcls, dim, vocab, n)))

        def acc():
            api.check(L.q4_memset(pd.ptr, 0, 4))
            api.verify_accept(rows, vocab, vocab, [5] * D, x, dim, lo, xo, ring, ph, pd)
        res["pass_ms_by_positions"][str(n)] = {"pass_ms": spread(ms[1:]), "classifier_ms": spread(cls), "accept_ms": spread(launches_ms(acc)),
                                               "steps_ms": round(n * step_ms, 3)}
        print(n, res["pass_ms_by_positions"][str(n)], flush=True)

    # (c) the bounds
    res["bounds"] = {}
    for D in (1, 3, 7):
        t.set_speculative(draft=D, ngram=3, min=1)
        row = {}
        for kind, fn in (("all_accepted", lambda ring, room: R[len(ring):len(ring) + room]),
                         ("none_accepted", lambda ring, room: [wrong(R[len(ring)], vocab)] + [int(v) for v in R[len(ring) + 1:len(ring) + room]])):
            t.set_drafter(fn)
            before = t.spec_stats()
            tps = tokens_per_s(t, reps)
            after = t.spec_stats()
            assert np.array_equal(t.generate_ids(PROMPT_IDS, STEPS)[0], R), "the speculative run's tokens differ from the run without it"
            row[kind] = {"tokens_per_s": spread(tps), "passes_per_run": (after[0] - before[0]) // (reps + 1),
                         "accepted_per_run": (after[2] - before[2]) // (reps + 1)}
        # a pass of D drafts takes 1 / tps(none) and emits 1 + a tokens; steps take 1 / tps(off) each
        pass_ms = 1e3 / row["none_accepted"]["tokens_per_s"]["median"]
        row["pass_ms"] = round(pass_ms, 4)
        row["break_even_accepted_per_pass"] = round(pass_ms / step_ms - 1.0, 3)
        row["break_even_share_of_drafts"] = round((pass_ms / step_ms - 1.0) / D, 3)
        row["speedup_all_accepted"] = round(row["all_accepted"]["tokens_per_s"]["median"] / statistics.median(off), 3)
        res["bounds"][str(D)] = row
        print(D, row, flush=True)
    t.set_drafter(None)

    # (d) the built-in drafter
    res["builtin"] = {}
    for name, kw in (("draft=4,ngram=3,min=2", dict(draft=4, ngram=3, min=2)), ("draft=7,ngram=3,min=1", dict(draft=7, ngram=3, min=1))):
        t.set_speculative(**kw)
        before = t.spec_stats()
        tps = tokens_per_s(t, reps)
        after = t.spec_stats()
        res["builtin"][name] = {"tokens_per_s": spread(tps), "per_run": [(a - b) // (reps + 1) for a, b in zip(after, before)],
                                "distinct_tokens": len(set(R.tolist()))}
        print(name, res["builtin"][name], flush=True)
    t.set_speculative(draft=0)
    res["off_again_tokens_per_s"] = spread(tokens_per_s(t, reps))
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speculative_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "off":
        return child_off(a.model, a.reps)
    res = {"model": a.model, "steps": STEPS, "repeats": a.reps}
    if a.parent_lib:
        res["off_against_parent"] = {"parent": [], "change": []}
        for _ in range(3):
            for who, lib in (("parent", a.parent_lib), ("change", None)):
                env = dict(os.environ)
                if lib:
                    env["Q4_LIB_OVERRIDE"] = lib
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "off", "--model", a.model, "--reps", str(a.reps)], env=env,
                                     capture_output=True, text=True, timeout=600, check=True).stdout
                res["off_against_parent"][who].append(spread(json.loads(out.strip().splitlines()[-1])["tokens_per_s"]))
                print(who, res["off_against_parent"][who][-1], flush=True)
    res.update(measure(a.model, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
