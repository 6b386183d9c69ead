#!/usr/bin/env python3
"""Several prompt positions of a slot per batch pass (q4_batch_set_prefill; csrc/q4_batch.hip) measured on the flagship geometry, 7B on
one GPU. Writes profiles/batch_prefill_bench.json (or the path given with --out):
  (a) time to first token of ONE slot alone, prompts of 8 / 64 / 250 tokens: q4_batch_open plus the passes up to the first generated token at cap 1 and at
      cap 8, and beside them the model's own sequence ingesting the same prompt to its first token (q4_generate_ids: eight-row prompt passes), one process;
  (b) an arrival: three slots decode and a fourth opens on a 250-token prompt, caps 1 / 4 / 8 -- the newcomer's time to first token and the milliseconds
      per pass (= the decoders' per-token latency) while it ingests, beside the three decoders' pass with nobody arriving;
  (c) the run form of the split-context attention: a lone slot restored at position 2000 inside a long prompt at cap 5, so every pass is one five-row
      run; milliseconds per pass in the run form against the same passes in the row form (five one-row blocks per head and chunk), same process --
      needs the profiling build's q4_set_batch_run_form, so this part runs in a child process on libllama2_q4_prof.so;
  (d) unchanged behaviour against another build (--parent-lib: the parent commit's libllama2_q4.so): tools/bench_batch.py's generations with the cap
      never set, and bench.py with no batch created, three alternating processes each; "inside" says whether this build's median lies in the parent's
      [min, max].
Every figure of (a) - (c) is the median of --reps measurements with [min, max] behind a warm-up run of the same shape. Every child process runs under a
time limit of its own; one that fails ends the tool.
    tools/bench_batch_prefill.py [--out FILE] [--parent-lib PATH] [--model 7b] [--reps 5] [--parts abcd]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_batch import open_model, spread      # noqa: E402

DEPTH, RUN_ROWS, RUN_PASSES = 2000, 5, 8


def wall(api, fn):
    api.synchronize()
    t0 = time.perf_counter()
    fn()
    api.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def passes_to_first_token(n_prompt, rows):
    return (n_prompt + rows - 1) // rows


def measure(model, reps, parts):
    import numpy as np
    res = {}
    rng = np.random.default_rng(11)
    api, L, t = open_model(model)
    vocab, S = t.config.vocab_size, t.config.seq_len
    text = [1] + [int(x) for x in rng.integers(3, vocab, size=S - 1)]

    def timed(fn):
        fn()
        return spread([fn() for _ in range(reps)])

    if "a" in parts:
        res["first_token_one_slot"] = {}
        batch = api.Batch(t, 1)
        for n in (8, 64, 250):
            row = {}
            for cap in (1, 8):
                batch.set_prefill(cap)
                passes = passes_to_first_token(n, cap)

                def run():
                    got = []
                    ms = wall(api, lambda: (batch.open(0, text[:n]), got.append(batch.generate(passes))))
                    assert got[0].shape[0] == passes and got[0][-1, 0] >= 0 and (got[0][:-1, 0] == -1).all()
                    batch.close(0)
                    return ms
                row["cap_%d" % cap] = {"passes": passes, "ms": timed(run)}
            row["own_sequence_ms"] = timed(lambda: wall(api, lambda: t.generate_ids(text[:n], n)))
            res["first_token_one_slot"][str(n)] = row
            print("(a)", n, row, flush=True)
        batch.delete()

    if "b" in parts:
        res["arrival"] = {"decoders": 3, "newcomer_prompt": 250}
        n = 250
        batch = api.Batch(t, 4)

        def settle():
            for slot in range(3):
                batch.open(slot, text[:8], seed=slot + 1)
            batch.generate(20)

        def done(n_open):
            for slot in range(n_open):
                batch.close(slot)

        def alone():
            settle()
            ms = wall(api, lambda: batch.generate(50)) / 50
            done(3)
            return ms
        res["arrival"]["nobody_arrives_ms_per_pass"] = timed(alone)
        for cap in (1, 4, 8):
            batch.set_prefill(cap)
            passes = passes_to_first_token(n, min(cap, 5))       # four open slots: four spare rows, so at most five rows for the newcomer
            one = []

            def run():
                settle()
                got = []
                ms = wall(api, lambda: (batch.open(3, text[:n]), got.append(batch.generate(passes))))
                assert got[0][-1, 3] >= 0 and (got[0][:-1, 3] == -1).all() and (got[0][:, :3] >= 0).all()
                done(4)
                one.append(ms / passes)
                return ms
            first = timed(run)
            res["arrival"]["cap_%d" % cap] = {"passes": passes, "newcomer_first_token_ms": first, "decoders_ms_per_token_meanwhile": spread(one[1:])}
            print("(b) cap", cap, res["arrival"]["cap_%d" % cap], flush=True)
        batch.delete()

    if "c" in parts:
        assert hasattr(L, "q4_set_batch_run_form"), "part (c) needs the profiling build (Q4_PROFILING_BUILD=1)"
        n_prompt = DEPTH + RUN_ROWS * RUN_PASSES + 8
        t.generate_ids(text[:DEPTH + 1], DEPTH + 1)
        snap = t.snapshot(DEPTH)
        batch = api.Batch(t, 1, prefill_rows=RUN_ROWS)
        row = {"position": DEPTH, "rows": RUN_ROWS, "passes_timed_together": RUN_PASSES}
        for name, on in (("run_form", 1), ("row_form", 0), ("run_form_again", 1)):
            L.q4_set_batch_run_form(on)

            def run():
                batch.restore(0, snap, text[:n_prompt])
                ms = wall(api, lambda: batch.generate(RUN_PASSES)) / RUN_PASSES
                assert batch.pos(0) == DEPTH + RUN_ROWS * RUN_PASSES
                batch.close(0)
                return ms
            row[name + "_ms_per_pass"] = timed(run)
        L.q4_set_batch_run_form(1)
        batch.delete()
        snap.close()
        res["run_form"] = row
        print("(c)", row, flush=True)
    t.close()
    return res


def child(args, env_extra, limit):
    env = dict(os.environ)
    env.update(env_extra)
    return subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=limit, check=True).stdout


def inside(change, parent):
    return {"change_median": round(statistics.median(change), 3), "parent_median": round(statistics.median(parent), 3), "parent_min": round(min(parent), 3),
            "parent_max": round(max(parent), 3), "inside": min(parent) <= statistics.median(change) <= max(parent), "change": change, "parent": parent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_prefill_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:                        # part (c), in a process of its own on the profiling build
        json.dump(measure(a.model, a.reps, "c"), open(a.child, "w"))
        return
    res = {"model": a.model, "repeats": a.reps}
    if os.path.exists(a.out):          # parts measured by an earlier call stay
        res.update(json.load(open(a.out)))

    def save():                        # behind every part: what was measured stays when a later part fails
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    if "d" in a.parts and a.parent_lib:      # first: the processes that must not see the cap, on a device nothing else of this tool has warmed
        parent = {"Q4_LIB_OVERRIDE": os.path.abspath(a.parent_lib)}
        runs = {"parent": {"bench": [], "batch": []}, "change": {"bench": [], "batch": []}}
        with tempfile.TemporaryDirectory() as d:
            for i in range(3):
                for who, env in (("parent", parent), ("change", {})):
                    out = child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--model", a.model], env, 300)
                    runs[who]["bench"].append(json.loads(out.strip().splitlines()[-1])["value"])
                    path = os.path.join(d, "%s_%d.json" % (who, i))
                    child([os.path.join(ROOT, "tools", "bench_batch.py"), "--parts", "a", "--reps", "3", "--model", a.model, "--out", path], env, 600)
                    runs[who]["batch"].append(json.load(open(path))["generation"])
                    print("(d)", who, i, runs[who]["bench"][-1], flush=True)
        d_res = {"bench_py_tokens_per_s": inside(runs["change"]["bench"], runs["parent"]["bench"])}
        for mode in ("greedy", "sampled_t0.5_p0.6"):
            for n in (1, 2, 4, 8):
                def pick(who):
                    return [g[mode]["slots_%d" % n]["ms_per_pass"]["median"] for g in runs[who]["batch"]]
                d_res["bench_batch_%s_slots_%d_ms_per_pass" % (mode, n)] = inside(pick("change"), pick("parent"))
        res["unchanged_against_parent"] = d_res
        save()
    if "c" in a.parts:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "c.json")
            print(child([os.path.abspath(__file__), "--child", path, "--model", a.model, "--reps", str(a.reps)], {"Q4_PROFILING_BUILD": "1"}, 600), end="", flush=True)
            res.update(json.load(open(path)))
        save()
    ab = "".join(p for p in "ab" if p in a.parts)
    if ab:
        res.update(measure(a.model, a.reps, ab))
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
