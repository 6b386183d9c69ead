"""What sequence snapshots cost and save (csrc/q4_snapshot.hip, csrc/q4_kv_copy.hip), on one MI355X from one process:

  for 7B fp16 and 7B FP8 at n_pos 128 / 512 / 2000, and 7B with a 16 K context (7b_16k) at n_pos 8000 / 16000:
    - the wall time to ingest n_pos prompt tokens one step each -- the only way to those rows without a snapshot;
    - q4_snapshot_new (the whole call: allocation, the copy launch, the synchronise) and q4_snapshot_restore (the copy launch alone, queued --batch
      at a time behind one synchronise), the bytes moved and bytes / time;
    - two yardsticks in the same run: the same arrays -- K, V and for FP8 the two exponent arrays -- moved by hipMemcpy2DAsync on the same stream (called
      from here through ctypes; the exponent arrays of the model are not reachable from outside, so buffers of their shape stand in), and a contiguous
      device-to-device torch copy of the same byte count (in a child process: torch brings its own HIP runtime).
  and, with --parent-lib (a libllama2_q4.so built from the parent commit), tokens/s of a plain greedy -n 256 run of this build and the parent's side
  by side through tools/ab.py: the decode step itself is unchanged.

Every timing is a host clock around work that ends in a stream synchronise; each figure is the median of --repeats batches, with the fastest and the
slowest batch beside it. Writes profiles/snapshot_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAN = (("7b", "fp16", (128, 512, 2000)), ("7b", "fp8", (128, 512, 2000)), ("7b_16k", "fp16", (8000, 16000)))
TORCH_CHILD = r'''
import json, sys, time, torch
out = {}
for n in map(int, sys.argv[3:]):
    a = torch.empty(n, dtype=torch.uint8, device="cuda"); b = torch.empty(n, dtype=torch.uint8, device="cuda")
    a.fill_(3); b.copy_(a); torch.cuda.synchronize()
    ts = []
    for _ in range(int(sys.argv[1])):
        t0 = time.perf_counter()
        for _ in range(int(sys.argv[2])): b.copy_(a)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / int(sys.argv[2]))
    out[str(n)] = sorted(ts)
    del a, b
print("RESULT " + json.dumps(out))
'''


def stats(per_op_seconds, nbytes=None):
    s = sorted(per_op_seconds)
    out = {"ms_median": round(1e3 * s[len(s) // 2], 4), "ms_best": round(1e3 * s[0], 4), "ms_worst": round(1e3 * s[-1], 4)}
    if nbytes:
        out["gb_per_s_median"] = round(nbytes / s[len(s) // 2] / 1e9, 1)
        out["gb_per_s_best"] = round(nbytes / s[0] / 1e9, 1)
    return out


def model_file(model_dir, name, synth):
    path = os.path.join(model_dir, "llama2_q4_synth_%s_seed20240229.bin" % name)
    geom = synth.GEOMETRIES[name]
    if os.path.exists(path) and os.path.getsize(path) == synth.model_bytes(geom):
        return path
    base = os.path.join(model_dir, "llama2_q4_synth_7b_seed20240229.bin")
    if name == "7b_16k" and os.path.exists(base):        # the same tensors from the same seed behind another header
        shutil.copyfile(base, path)
        with open(path, "r+b") as f:
            f.write(struct.pack("<7if", *geom))
        return path
    synth.write_model(path, geom)
    return path


def batches(repeats, batch, enqueue, sync):
    enqueue()
    sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(batch):
            enqueue()
        sync()
        out.append((time.perf_counter() - t0) / batch)
    return out


def measure_model(args, api, synth, hip, name, kv, n_list, res):
    import numpy as np
    t = api.Transformer(model_file(args.model_dir, name, synth), kv=kv)
    cfg = t.config
    kv_dim = cfg.dim * cfg.n_kv_heads // cfg.n_heads
    elem = 1 if kv == "fp8" else 2
    rng = np.random.default_rng(7)
    prompt = rng.integers(3, cfg.vocab_size, max(n_list), dtype=np.int32)
    prompt[0] = 1
    stream = api.lib().q4_get_stream()
    state = t.state.contents
    exp_stand_in = [api.DevBuf(nbytes=cfg.n_layers * cfg.n_kv_heads * cfg.seq_len) for _ in range(2)] if kv == "fp8" else []
    for n in n_list:
        row = {"model": name, "kv": kv, "n_pos": n}
        warm = n <= 2048                                                          # a first pass captures the graphs of every bin the timed one uses
        t.generate_ids(prompt[:n] if warm else prompt[:8], n if warm else 8)
        t0 = time.perf_counter()
        t.generate_ids(prompt[:n], n)
        row["ingest_seconds"] = round(time.perf_counter() - t0, 4)
        row["ingest_includes_graph_captures"] = not warm                          # (long contexts are ingested once: a few captures inside tens of seconds)
        assert t.pos() == n
        new_times = []
        for _ in range(args.repeats + 1):
            t0 = time.perf_counter()
            snap = t.snapshot(n)
            new_times.append(time.perf_counter() - t0)
            if len(new_times) <= args.repeats:
                snap.close()
        nbytes = snap.nbytes
        row["bytes"] = nbytes
        row["snapshot_new"] = stats(new_times[1:], nbytes)
        row["restore"] = stats(batches(args.repeats, args.batch, lambda: t.restore(snap), api.synchronize), nbytes)
        # yardstick 1: the same arrays by hipMemcpy2DAsync, cache -> a packed buffer
        packed = api.DevBuf(nbytes=nbytes)
        run, layer = n * kv_dim * elem, cfg.seq_len * kv_dim * elem
        parts = [(packed.ptr, run, state.key_cache, layer, run, cfg.n_layers), (packed.ptr + cfg.n_layers * run, run, state.value_cache, layer, run, cfg.n_layers)]
        at = 2 * cfg.n_layers * run
        for e in exp_stand_in:
            rows = cfg.n_layers * cfg.n_kv_heads
            parts.append((packed.ptr + at, n, e.ptr, cfg.seq_len, n, rows))
            at += rows * n
        assert at == nbytes

        def by_runtime():
            for dst, dpitch, src, spitch, width, height in parts:
                rc = hip.hipMemcpy2DAsync(C.c_void_p(dst), C.c_size_t(dpitch), C.c_void_p(src), C.c_size_t(spitch), C.c_size_t(width), C.c_size_t(height), 3,
                                          C.c_void_p(stream))
                if rc != 0:
                    raise RuntimeError("hipMemcpy2DAsync: %d" % rc)
        row["hipMemcpy2DAsync_calls"] = len(parts)
        row["hipMemcpy2DAsync"] = stats(batches(args.repeats, args.batch, by_runtime, api.synchronize), nbytes)
        packed.free()
        snap.close()
        res["rows"].append(row)
        print(json.dumps(row, sort_keys=True), flush=True)
    for e in exp_stand_in:
        e.free()
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--repeats", type=int, default=7, help="timed batches per figure")
    ap.add_argument("--batch", type=int, default=20, help="copies queued behind one synchronise")
    ap.add_argument("--only", default=None, help="model:kv:n_pos[,n_pos] instead of the full plan (a rehearsal on a small model)")
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so of the parent commit, run side by side through tools/ab.py")
    ap.add_argument("--limit", type=int, default=420, help="seconds for each child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.json"))
    args = ap.parse_args()

    from llama_cu_awq_amd import api, synth
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    try:                                                # (the runtime the library itself is linked against: already loaded)
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    plan = PLAN
    if args.only:
        m, kv, ns = args.only.split(":")
        plan = ((m, kv, tuple(int(x) for x in ns.split(","))),)
    res = {"device": api.device_info()[0], "repeats": args.repeats, "batch": args.batch, "rows": [],
           "note": "ms per copy; gb_per_s = snapshot bytes / time (the traffic is twice that: every byte is read and written)"}
    for name, kv, n_list in plan:
        measure_model(args, api, synth, hip, name, kv, n_list, res)
    L.q4_stream_synchronize()
    L.q4_set_stream(None)
    L.q4_stream_destroy(s)

    # yardstick 2: contiguous device-to-device torch copies of the same byte counts, in a child of its own
    sizes = sorted({r["bytes"] for r in res["rows"]})
    failed = False
    try:
        p = subprocess.run([sys.executable, "-c", TORCH_CHILD, str(args.repeats), str(args.batch)] + [str(n) for n in sizes], capture_output=True, text=True,
                           timeout=args.limit)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode == 0 and lines:
            got = json.loads(lines[-1][7:])
            for r in res["rows"]:
                r["torch_contiguous_copy"] = stats(got[str(r["bytes"])], r["bytes"])
        else:
            failed = True
            res["torch_contiguous_copy_error"] = "exit status %d: %s" % (p.returncode, p.stderr[-300:])
    except subprocess.TimeoutExpired:
        failed = True
        res["torch_contiguous_copy_error"] = "no result within %d s" % args.limit
    for r in res["rows"]:
        faster = min(r["hipMemcpy2DAsync"]["ms_median"], r.get("torch_contiguous_copy", {}).get("ms_median", float("inf")))
        r["restore_over_faster_yardstick"] = round(r["restore"]["ms_median"] / faster, 3)

    # the decode step, this build against the parent's (a failed child on the GPU: nothing more is started there)
    if args.parent_lib and not failed:
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab.py"), "7b", "256", "3", os.path.abspath(args.parent_lib), api.LIB_PATH],
                               capture_output=True, text=True, timeout=args.limit)
            rows = re.findall(r"^(\S+)\s+7b -n 256\s+best ([0-9.]+)\s+median of medians ([0-9.]+)\s+\(([0-9. ]+)\)", p.stdout, flags=re.M)
            if p.returncode == 0 and len(rows) == 2:
                res["decode_n256_tokens_per_s"] = {("parent" if i == 0 else "this_build"): {"best": float(b), "median_of_medians": float(m), "medians": [float(x) for x in ms.split()]}
                                                   for i, (_, b, m, ms) in enumerate(rows)}
            else:
                res["decode_n256_error"] = "exit status %d: %s" % (p.returncode, (p.stderr or p.stdout)[-300:])
        except subprocess.TimeoutExpired:
            res["decode_n256_error"] = "no result within %d s" % args.limit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
