#!/usr/bin/env python3
"""Log-probability records inside prompt and verify passes (q4_set_pass_logprobs; DESIGN.md 3.4 / 3.7 / 3.8 "With records") measured at 7B on the
benchmark's prompt. Writes profiles/pass_logprobs_bench.json (or the path given with --out):
  (a) scoring: q4_score_ids over 250 tokens, the switch off against on, ms per call, K = 0 and 5 (records switched on beforehand: the ring stays);
  (b) reset to first generated token for 64 and 250 prompt tokens with logprobs = 5, the switch off against on, and with records off beside them -- the
      gap between the last two is the classifier plus the record launch per pass;
  (c) speculation with records: -n 256 greedy with logprobs = 5 -- speculation off, and 7 drafts with every draft accepted and with none, the switch on;
      one verify pass of n = 2 .. 8 rows with records against the same pass without them;
  (d) nothing changed for everyone else: -n 256 greedy and -t 0.5 -p 0.6 with the switch off against another build of the library (--parent-lib: the
      parent commit's libllama2_q4.so), three processes of each, alternating.
Medians of --reps with [min, max]. tokens/s figures are the token loop's own (the clock bench.py reads); ms figures the host clock around a call that
synchronises in front and behind. The weights are synthetic.
    tools/bench_pass_logprobs.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5]"""
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
SAMPLED = dict(temperature=0.5, topp=0.6, seed=1)         # the CLI's defaults


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


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def tokens_per_s(t, reps, prompt=PROMPT_IDS, steps=STEPS, seed=None):
    out = []
    for i in range(reps + 1):                               # the first warms: graphs captured, scratch allocated
        if seed is not None:
            C.cast(t.sampler, C.POINTER(SamplerStruct)).contents.rng_state = seed
        out.append(t.generate_ids(prompt, steps)[1])
    return out[1:]


def child_off(model, reps, sampled):
    """one process: every switch at its default, tokens/s of `reps` generations"""
    api, _ = open_library()
    t = api.Transformer(model_path(model), **(SAMPLED if sampled else {}))
    print(json.dumps({"tokens_per_s": tokens_per_s(t, reps, seed=SAMPLED["seed"] if sampled else None)}))
    t.close()


def wrong(tok, vocab):
    w = (int(tok) + 1) % vocab
    return w + 1 if w == 2 else w


def measure(model, reps):
    import numpy as np
    api, L = open_library()
    path = model_path(model)
    res = {}
    rng = np.random.default_rng(7)
    t = api.Transformer(path)
    vocab = t.config.vocab_size

    def timed(fn):
        fn()
        out = []
        for _ in range(reps):
            api.synchronize()
            t0 = time.perf_counter()
            fn()
            out.append(1e3 * (time.perf_counter() - t0))
        return out

    # (a) scoring
    res["score_250_tokens_ms"] = {}
    ids = [1] + [int(x) for x in rng.integers(3, vocab, size=250)]
    for k in (0, 5):
        t.set_logprobs(k)
        row = {}
        for on in (False, True):
            t.set_pass_logprobs(on)
            before = api.prompt_passes()
            row["switch_on" if on else "switch_off"] = spread(timed(lambda: t.score_ids(ids)))
            row["passes_per_call_on" if on else "passes_per_call_off"] = (api.prompt_passes() - before) // (reps + 1)
        row["ratio"] = round(row["switch_off"]["median"] / row["switch_on"]["median"], 3)
        res["score_250_tokens_ms"]["K=%d" % k] = row
        print("score", k, row, flush=True)

    # (b) reset to first generated token
    def first_token_ms(prompt):
        steps = len(prompt) + 1      # the loop's clock stops once the step BEHIND the one it queued last has ended: queue one more
        t.generate_ids(prompt, steps)
        return [1e3 * t.generate_ids(prompt, steps)[3] for _ in range(reps)]

    res["first_token_ms"] = []
    for n in (64, 250):
        prompt = [1] + [int(x) for x in rng.integers(3, vocab, size=n - 1)]
        row = {"prompt_tokens": n}
        t.set_logprobs(5)
        t.set_pass_logprobs(False)
        row["records_switch_off"] = spread(first_token_ms(prompt))
        t.set_pass_logprobs(True)
        before = api.prompt_passes()
        row["records_switch_on"] = spread(first_token_ms(prompt))
        passes = (api.prompt_passes() - before) // (reps + 1)
        t.set_logprobs(None)
        row["no_records"] = spread(first_token_ms(prompt))
        row["passes"] = passes
        row["ratio_with_records"] = round(row["records_switch_off"]["median"] / row["records_switch_on"]["median"], 3)
        row["records_cost_per_pass_ms"] = round((row["records_switch_on"]["median"] - row["no_records"]["median"]) / max(passes, 1), 4)
        res["first_token_ms"].append(row)
        print("first token", row, flush=True)

    # (c) speculation with records
    t.set_logprobs(5)
    t.set_pass_logprobs(False)
    off = tokens_per_s(t, reps)
    R = t.generate_ids(PROMPT_IDS, STEPS)[0].copy()
    assert 2 not in R[1:].tolist()
    step_ms = 1e3 / statistics.median(off)
    spec = {"records_no_speculation_tokens_per_s": spread(off)}
    t.set_pass_logprobs(True)
    t.set_speculative(draft=7, ngram=3, min=1)
    for kind, fn in (("all_accepted", lambda ring, room: R[len(ring):len(ring) + room]),
                     ("none_accepted", lambda ring, room: [wrong(R[len(ring)], vocab)] + [int(v) for v in R[len(ring) + 1:len(ring) + room]])):
        t.set_drafter(fn)
        before = t.spec_stats()
        tps = tokens_per_s(t, reps)
        after = t.spec_stats()
        assert np.array_equal(t.generate_ids(PROMPT_IDS, STEPS)[0], R), "the speculative run's tokens differ from the run without it"
        spec[kind] = {"tokens_per_s": spread(tps), "passes_per_run": (after[0] - before[0]) // (reps + 1), "accepted_per_run": (after[2] - before[2]) // (reps + 1)}
    spec["speedup_all_accepted"] = round(spec["all_accepted"]["tokens_per_s"]["median"] / statistics.median(off), 3)
    t.set_drafter(None)
    t.set_speculative(draft=0)
    res["speculation_K5"] = spec
    print("speculation", spec, flush=True)
    # one verify pass at position 20 by the host clock around the primitive (it synchronises in front and behind), with records and without
    res["verify_pass_ms_by_rows"] = {}
    for n in range(2, 9):
        D = n - 1
        row = {}
        for name, k in (("records_K5", 5), ("no_records", None)):
            t.set_logprobs(k)
            ms = []
            for _ in range(reps + 1):
                t.generate_ids(PROMPT_IDS, 20)
                api.synchronize()
                t0 = time.perf_counter()
                got = t.verify([int(v) for v in R[21:21 + D]])
                ms.append(1e3 * (time.perf_counter() - t0))
                assert got is not None and got[1] == D, "the pass is not admitted, or the run's own continuation was not accepted"
            row[name] = spread(ms[1:])
        row["added_ms"] = round(row["records_K5"]["median"] - row["no_records"]["median"], 4)
        row["steps_with_records_ms"] = round(n * step_ms, 3)
        res["verify_pass_ms_by_rows"][str(n)] = row
        print(n, row, flush=True)
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_logprobs_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child_off(a.model, a.reps, a.child == "sampled")
    res = {"model": a.model, "steps": STEPS, "repeats": a.reps}
    if a.parent_lib:
        res["off_against_parent"] = {}
        for mode in ("greedy", "sampled"):
            row = {"parent": [], "change": []}
            for _ in range(3):
                for who, lib in (("parent", a.parent_lib), ("change", None)):
                    env = dict(os.environ)
                    if lib:
                        env["Q4_LIB_OVERRIDE"] = lib
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--model", a.model, "--reps", str(a.reps)], env=env,
                                         capture_output=True, text=True, timeout=600, check=True).stdout
                    row[who].append(spread(json.loads(out.strip().splitlines()[-1])["tokens_per_s"]))
                    print(mode, who, row[who][-1], flush=True)
            p = [r["median"] for r in row["parent"]]
            c = [r["median"] for r in row["change"]]
            row["parent_spread"] = round(max(p) - min(p), 3)
            row["change_minus_parent_medians"] = round(statistics.median(c) - statistics.median(p), 3)
            row["change_inside_parent_spread"] = bool(min(p) <= statistics.median(c) <= max(p))
            res["off_against_parent"][mode] = row
    res.update(measure(a.model, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
