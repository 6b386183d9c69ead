"""What a context shift costs (csrc/q4_kv_shift.hip, q4_shift_context), on one MI355X from one process:

  q4_shift_context(n_pos, keep, discard) at 7B fp16 and 7B FP8 (2048, 4, 1022) and (2048, 4, 1), mistral7b (2048, 4, 1022), 7b_16k (16384, 4, 8190):
  the whole call (the in-place launch, the position, the hand-off words, the synchronise), the K / V bytes it moves and the GB/s that is, read plus
  write. Two yardsticks in the same run:
    - re-ingesting the n_pos - discard surviving tokens step by step: the only way on a sequence has without the shift;
    - the same rows moved out to a scratch buffer and back by q4_copy_runs launches (two per tensor: K, then V) -- the overlap-free way, where a
      scratch of the moved rows' size can be allocated at all (recorded when it cannot).

Every timing is a host clock around work that ends in a stream synchronise, after a first untimed pass of the same shape; each figure is the median
of --repeats batches with the fastest and the slowest beside it. Between two timed shifts the position is put back with q4_resume_sequence (not timed).
Writes profiles/context_shift_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PLAN = (("7b", "fp16", ((2048, 4, 1022), (2048, 4, 1))), ("7b", "fp8", ((2048, 4, 1022), (2048, 4, 1))), ("mistral7b", "fp16", ((2048, 4, 1022),)),
        ("7b_16k", "fp16", ((16384, 4, 8190),)))


def stats(seconds, nbytes=None):
    s = sorted(seconds)
    out = {"ms_median": round(1e3 * s[len(s) // 2], 4), "ms_best": round(1e3 * s[0], 4), "ms_worst": round(1e3 * s[-1], 4)}
    if nbytes:
        out["gb_per_s_median"] = round(nbytes / s[len(s) // 2] / 1e9, 1)
        out["gb_per_s_best"] = round(nbytes / s[0] / 1e9, 1)
    return out


def measure_model(args, api, synth, name, kv, cases, res):
    import numpy as np
    from bench_snapshot import model_file
    t = api.Transformer(model_file(args.model_dir, name, synth), kv=kv)
    cfg = t.config
    kv_dim = cfg.dim * cfg.n_kv_heads // cfg.n_heads
    elem = 1 if kv == "fp8" else 2
    rng = np.random.default_rng(7)
    tokens = rng.integers(3, cfg.vocab_size, cfg.seq_len + 1, dtype=np.int32)
    tokens[0] = 1
    state = t.state.contents
    filled = 0
    for n_pos, keep, D in cases:
        M = n_pos - keep - D
        row = {"model": name, "kv": kv, "n_pos": n_pos, "keep": keep, "discard": D, "rows_moved": M}
        # yardstick 1 (and real rows under the timed shifts): ingest the surviving tokens; a first pass captures the graphs of every bin
        survive = n_pos - D
        if filled < survive:
            t.generate_ids(tokens[:survive], survive)
        t0 = time.perf_counter()
        t.generate_ids(tokens[:survive], survive)
        row["reingest_seconds"] = round(time.perf_counter() - t0, 4)
        row["reingest_tokens"] = survive
        filled = max(filled, survive)
        moved = 2 * cfg.n_layers * M * kv_dim * elem + (2 * cfg.n_layers * cfg.n_kv_heads * M if kv == "fp8" else 0)
        row["bytes_moved"] = moved

        def one_shift():
            t.resume(tokens[:n_pos + 1], n_pos)                 # the position back at n_pos (not timed; the rows' values do not matter to the clock)
            t0 = time.perf_counter()
            t.shift_context(keep, D, n_pos=n_pos)
            return time.perf_counter() - t0
        one_shift()
        one_shift()
        per_batch = [sum(one_shift() for _ in range(args.batch)) / args.batch for _ in range(args.repeats)]
        row["shift_context"] = stats(per_batch, 2 * moved)       # read plus write
        row["reingest_over_shift"] = round(row["reingest_seconds"] / (row["shift_context"]["ms_median"] * 1e-3), 1)

        # yardstick 2: out to a scratch buffer and back, two q4_copy_runs launches per tensor
        run, layer = M * kv_dim * elem, cfg.seq_len * kv_dim * elem
        try:
            scratch = api.DevBuf(nbytes=cfg.n_layers * run)
        except api.Q4Error as e:
            scratch = None
            row["scratch_copy_error"] = "no scratch of %d bytes: %s" % (cfg.n_layers * run, e)
        if scratch is not None:
            L = api.lib()

            def out_and_back():
                for cache in (state.key_cache, state.value_cache):
                    api.check(L.q4_copy_runs(scratch.ptr, cache + (keep + D) * kv_dim * elem, cfg.n_layers, run, layer, run))
                    api.check(L.q4_copy_runs(cache + keep * kv_dim * elem, scratch.ptr, cfg.n_layers, layer, run, run))
            out_and_back()
            api.synchronize()
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for _ in range(args.batch):
                    out_and_back()
                api.synchronize()
                ts.append((time.perf_counter() - t0) / args.batch)
            row["scratch_bytes"] = cfg.n_layers * run
            row["scratch_out_and_back"] = stats(ts, 4 * 2 * cfg.n_layers * run)      # every row is read and written twice
            row["scratch_over_shift"] = round(row["scratch_out_and_back"]["ms_median"] / row["shift_context"]["ms_median"], 3)
            scratch.free()
        res["rows"].append(row)
        print(json.dumps(row, sort_keys=True), flush=True)
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--repeats", type=int, default=7, help="timed batches per figure")
    ap.add_argument("--batch", type=int, default=5, help="operations per batch")
    ap.add_argument("--only", default=None, help="model:kv:n_pos,keep,discard instead of the full plan (a rehearsal on a small model)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_shift_bench.json"))
    args = ap.parse_args()

    from llama_cu_awq_amd import api, synth
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    plan = PLAN
    if args.only:
        m, kv, case = args.only.split(":")
        plan = ((m, kv, (tuple(int(x) for x in case.split(",")),)),)
    res = {"device": api.device_info()[0], "repeats": args.repeats, "batch": args.batch, "rows": [],
           "note": "shift_context: ms per call, GB/s over bytes read plus bytes written; scratch_out_and_back: four q4_copy_runs launches (K and V, out "
                   "and back); reingest: generate_ids over the surviving tokens, graphs already captured"}
    for name, kv, cases in plan:
        measure_model(args, api, synth, name, kv, cases, res)
    L.q4_stream_synchronize()
    L.q4_set_stream(None)
    L.q4_stream_destroy(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
