#!/usr/bin/env python3
"""Verify passes under the temperature / top-p sampler (q4_set_speculative_sampled) measured on the flagship workload as the CLI samples
it by default: 7B, -n 256, -t 0.5 -p 0.6, the benchmark's prompt. Writes profiles/speculative_sampled_bench.json (or the path given with --out):
  (a) the feature off against another build of the library (--parent-lib: the parent commit's libllama2_q4.so): three processes of each, alternating;
  (b) one sampled pass of n = 2 .. 8 rows, the greedy pass beside it, and the launches only the sampled pass has -- the row softmax, the row search, the
      accept on given tokens -- alone;
  (c) the bounds: a drafter that returns the sampled run's own continuation (every draft accepted) and one whose first token is wrong (none), at 1, 3, 7
      drafts, and from them the accepted drafts per pass at which a pass breaks even.
Every tokens/s figure is the token loop's own (timed tokens over its seconds, the clock bench.py reads), median of --reps generations with min and max.
Acceptance on real checkpoints is not measured here: the weights are synthetic.
    tools/bench_speculative_sampled.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5]"""
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
TEMPERATURE, TOPP, SEED = 0.5, 0.6, 1                     # the CLI's defaults


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
    return api, L, api.Transformer(path, temperature=TEMPERATURE, topp=TOPP, seed=SEED)


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def reseed(t):
    """every generation samples with the same coin stream: the run is the same run"""
    C.cast(t.sampler, C.POINTER(SamplerStruct)).contents.rng_state = SEED


def generate(t, steps=STEPS):
    reseed(t)
    return t.generate_ids(PROMPT_IDS, steps)


def tokens_per_s(t, reps):
    generate(t)                                                 # warm: graphs captured, scratch allocated
    return [generate(t)[1] for _ in range(reps)]


def child_off(model, reps):
    """one process: the feature off (a build without it has nothing to switch), tokens/s of `reps` sampled generations"""
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
    res = {"temperature": TEMPERATURE, "topp": TOPP, "seed": SEED}
    off = tokens_per_s(t, reps)
    R = generate(t)[0].copy()
    assert 2 not in R[1:].tolist(), "the sampled run meets an EOS: choose another seed"
    res["off_tokens_per_s"] = spread(off)
    step_ms = 1e3 / statistics.median(off)

    # the greedy continuation from position 20 of the same prompt, for the greedy pass beside the sampled one
    g = api.Transformer(t_path(model))
    G = g.generate_ids(PROMPT_IDS, STEPS)[0].copy()

    # (b) one pass at position 20, by the host clock around the primitive (it synchronises in front and behind); the launches only the sampled pass
    # has, alone, twenty back to back between two synchronisations, on rows of the model's vocabulary
    res["pass_ms_by_rows"] = {}
    rows_host = (np.random.default_rng(1).standard_normal((8, vocab)) * 2.0).astype(np.float16)
    rows = api.DevBuf(rows_host)
    x = api.DevBuf(np.random.default_rng(1).standard_normal((8, dim)).astype(np.float16))
    lo, xo = api.DevBuf(nbytes=vocab * 2), api.DevBuf(nbytes=dim * 2)
    ring, ph, pd, win = api.DevBuf(nbytes=64 * 4), api.DevBuf(nbytes=16), api.DevBuf(nbytes=16), api.DevBuf(nbytes=32)

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

    t.set_speculative(draft=0, sampled=True)
    for n in range(2, 9):
        D = n - 1
        ms, gms = [], []
        for _ in range(reps + 1):
            generate(t, 20)
            api.synchronize()
            t0 = time.perf_counter()
            got = t.verify_sampled([int(v) for v in R[21:21 + D]])
            ms.append(1e3 * (time.perf_counter() - t0))
            assert got is not None and got[1] == D, "the sampled pass is not admitted, or the run's own continuation was not accepted"
            g.generate_ids(PROMPT_IDS, 20)
            api.synchronize()
            t0 = time.perf_counter()
            got = g.verify([int(v) for v in G[21:21 + D]])
            gms.append(1e3 * (time.perf_counter() - t0))
            assert got is not None and got[1] == D

        def sample_rows():          # (the rows become probabilities after the first call: the launches' work does not depend on the values)
            api.verify_sample_rows(t.sampler, rows, vocab, n, [0.37] * n, win)

        def accept():
            api.check(L.q4_memset(pd.ptr, 0, 4))
            api.verify_accept_tokens(rows, vocab, vocab, [5] * D, win, x, dim, lo, xo, ring, ph, pd)

        def accept_greedy():
            api.check(L.q4_memset(pd.ptr, 0, 4))
            api.verify_accept(rows, vocab, vocab, [5] * D, x, dim, lo, xo, ring, ph, pd)
        row = {"sampled_pass_ms": spread(ms[1:]), "greedy_pass_ms": spread(gms[1:]), "sampler_rows_ms": spread(launches_ms(sample_rows)),
               "accept_tokens_ms": spread(launches_ms(accept)), "accept_greedy_ms": spread(launches_ms(accept_greedy)), "steps_ms": round(n * step_ms, 3)}
        row["sampled_minus_greedy_ms"] = round(row["sampled_pass_ms"]["median"] - row["greedy_pass_ms"]["median"], 4)
        row["new_launches_share_of_pass"] = round((row["sampler_rows_ms"]["median"] + row["accept_tokens_ms"]["median"]) / row["sampled_pass_ms"]["median"], 4)
        res["pass_ms_by_rows"][str(n)] = row
        print(n, row, flush=True)
    g.close()

    # (c) the bounds
    res["bounds"] = {}
    for D in (1, 3, 7):
        t.set_speculative(draft=D, ngram=3, min=1, sampled=True)
        row = {}
        for kind, fn in (("all_accepted", lambda ring, room: R[len(ring):len(ring) + room]),
                         ("none_accepted", lambda ring, room: [wrong(R[len(ring)], vocab)] + [int(v) for v in R[len(ring) + 1:len(ring) + room]])):
            t.set_drafter(fn)
            before = t.spec_stats()
            tps = tokens_per_s(t, reps)
            after = t.spec_stats()
            assert np.array_equal(generate(t)[0], R), "the speculative run's tokens differ from the run without it"
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
    t.set_speculative(draft=0)
    res["off_again_tokens_per_s"] = spread(tokens_per_s(t, reps))
    t.close()
    return res


def t_path(model):
    return os.path.join(os.environ.get("Q4_MODEL_DIR", "/tmp"), "llama2_q4_synth_%s_seed20240229.bin" % model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speculative_sampled_bench.json"))
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
        p = [r["median"] for r in res["off_against_parent"]["parent"]]
        c = [r["median"] for r in res["off_against_parent"]["change"]]
        res["off_against_parent"]["change_inside_parent_spread"] = bool(min(p) <= statistics.median(c) <= max(p))
    res.update(measure(a.model, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
