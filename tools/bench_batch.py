#!/usr/bin/env python3
"""Batched decoding (q4_batch_*; csrc/q4_batch.hip) measured on the flagship geometry, 7B on one GPU, against the solo steps of the SAME
process. Writes profiles/batch_bench.json (or the path given with --out):
  (a) aggregate and per-slot tokens/s at 1, 2, 4 and 8 slots, greedy and at temperature 0.5 / top-p 0.6: every slot an 8-token prompt and 247 generated
      tokens (254 passes, positions 0 .. 253), the host clock around q4_batch_generate (it synchronises at its end); the solo figure is the same 254
      positions through q4_generate_ids by the same clock, and the token loop's own tokens/s beside it;
  (b) one pass's milliseconds by row count (1 .. 8) at positions 30, 300 and 2000 -- the slots restored there from a snapshot of the model's own sequence,
      eight passes timed together -- and the solo step there (eight steps of a run resumed at the position);
  (c) bench.py in three alternating processes each of this build and of another one (--parent-lib: the parent commit's libllama2_q4.so), no batch created.
Every figure is the median of --reps measurements with [min, max]. Every child process runs under a time limit of its own; one that fails ends the tool.
    tools/bench_batch.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5] [--parts abc]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT, GENERATED = 8, 247
PASSES = PROMPT - 1 + GENERATED


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def open_model(model, temperature=0.0, topp=0.9):
    import ctypes as C
    from llama_cu_awq_amd import api, synth
    L = api.lib()
    api.check(L.q4_set_device(0))
    if not L.q4_get_stream():
        s = C.c_void_p()
        api.check(L.q4_stream_create(C.byref(s)))
        L.q4_set_stream(s)
    path = os.path.join(os.environ.get("Q4_MODEL_DIR", "/tmp"), "llama2_q4_synth_%s_seed20240229.bin" % model)
    if not (os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(synth.geometry(model))):
        synth.write_model(path, model)
    return api, L, api.Transformer(path, temperature=temperature, topp=topp)


def measure(model, reps, parts):
    import numpy as np
    res = {}
    rng = np.random.default_rng(7)

    def wall(fn):
        api.synchronize()
        t0 = time.perf_counter()
        fn()
        api.synchronize()
        return time.perf_counter() - t0

    # (a) whole generations
    if "a" in parts:
        res["generation"] = {"prompt_tokens": PROMPT, "generated_tokens": GENERATED, "passes": PASSES}
        for mode, temperature, topp in (("greedy", 0.0, 0.9), ("sampled_t0.5_p0.6", 0.5, 0.6)):
            api, L, t = open_model(model, temperature, topp)
            vocab = t.config.vocab_size
            prompts = [[1] + [int(x) for x in rng.integers(3, vocab, size=PROMPT - 1)] for _ in range(8)]
            row = {}
            t.generate_ids(prompts[0], PASSES)
            # (the solo runs share one Sampler, whose coin stream goes on from run to run, while a slot is reseeded by every open: the sampled runs differ
            # in their tokens, not in what a token costs)
            secs, loop = [], []
            for _ in range(reps):
                got = []
                secs.append(wall(lambda: got.append(t.generate_ids(prompts[0], PASSES))))
                loop.append(got[0][1])
            row["solo"] = {"tokens_per_s": spread([GENERATED / s for s in secs]), "token_loop_tokens_per_s": spread(loop)}
            for n in (1, 2, 4, 8):
                batch = api.Batch(t, n)

                def run():
                    for slot in range(n):
                        batch.open(slot, prompts[slot], seed=slot + 1)
                    s = wall(lambda: batch.generate(PASSES))
                    for slot in range(n):
                        assert batch.pos(slot) == PASSES
                        batch.close(slot)
                    return s
                run()
                secs = [run() for _ in range(reps)]
                row["slots_%d" % n] = {"aggregate_tokens_per_s": spread([n * GENERATED / s for s in secs]), "per_slot_tokens_per_s": spread([GENERATED / s for s in secs]),
                                       "ms_per_pass": spread([1e3 * s / PASSES for s in secs])}
                batch.delete()
                print("(a)", mode, n, row["slots_%d" % n], flush=True)
            for n in (2, 8):
                row["slots_%d_over_solo" % n] = round(row["slots_%d" % n]["aggregate_tokens_per_s"]["median"] / row["solo"]["tokens_per_s"]["median"], 3)
            res["generation"][mode] = row
            print("(a)", mode, "solo", row["solo"], flush=True)
            t.close()

    # (b) one pass by row count at depth, and the solo step there
    if "b" in parts:
        api, L, t = open_model(model)
        vocab, S = t.config.vocab_size, t.config.seq_len
        text = [1] + [int(x) for x in rng.integers(3, vocab, size=S - 1)]
        res["pass_at_depth"] = {}
        K = 8
        for p in (30, 300, 2000):
            at = {}
            t.generate_ids(text[:p + 1], p + 1)               # rows [0, p] of `text` in place: the snapshot's, and the resumed solo runs'
            snap = t.snapshot(p)
            t.generate_ids_from(text[:p + 1], p + K, p)       # K generating steps from position p (a longer prompt would be taken by a prompt pass)
            at["solo_step_ms"] = spread([1e3 * wall(lambda: t.generate_ids_from(text[:p + 1], p + K, p)) / K for _ in range(reps)])
            batch = api.Batch(t, 8)
            for n in range(1, 9):
                def run():
                    for slot in range(n):
                        batch.restore(slot, snap, text[:p + 1], seed=slot + 1)
                    s = wall(lambda: batch.generate(K))
                    for slot in range(n):
                        batch.close(slot)
                    return 1e3 * s / K
                run()
                at["rows_%d_pass_ms" % n] = spread([run() for _ in range(reps)])
            batch.delete()
            snap.close()
            res["pass_at_depth"][str(p)] = at
            print("(b) position", p, at, flush=True)
        t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    res = {"model": a.model, "repeats": a.reps}
    if os.path.exists(a.out):          # parts measured by an earlier call stay
        res.update(json.load(open(a.out)))
    if "c" in a.parts and a.parent_lib:      # first: the processes that must not see a batch, on a device nothing else of this tool has warmed
        res["bench_py_no_batch"] = {"parent": [], "change": []}
        for _ in range(3):
            for who, lib in (("parent", a.parent_lib), ("change", None)):
                env = dict(os.environ)
                if lib:
                    env["Q4_LIB_OVERRIDE"] = os.path.abspath(lib)
                out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--model", a.model],
                                     env=env, capture_output=True, text=True, timeout=300, check=True).stdout
                line = json.loads(out.strip().splitlines()[-1])
                res["bench_py_no_batch"][who].append({"tokens_per_s": line["value"], "per_generation": line.get("tok_s_per_generation")})
                print("(c)", who, line["value"], flush=True)
    if set(a.parts) & set("ab"):
        res.update(measure(a.model, a.reps, a.parts))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
