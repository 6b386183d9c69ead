"""What RoPE scaling costs (q4_set_rope_scaling), on one MI355X:

  tokens/s at 7B `-n 256` greedy, three configurations in fresh child processes, interleaved, `--rounds` (3) processes each: the parent commit's
  library (`--parent-lib`, unscaled), this build unscaled, this build with Llama-3.1's setting (llama3, factor 8, low 1, high 4, orig 8192). Each
  process runs one warm and four timed generations and reports their median. The decode step's launches do not change with the setting -- every
  rotation reads the model's table -- so the yardstick is the parent's own spread, max - min of its medians: a column further away than that needs an
  explanation.

  the table's build time at seq_len 2048 and 131072 (1 MB and 64 MB of table at head size 128), unscaled and scaled, as q4_build_transformer reports
  it under Q4_DEBUG_ROPE=1 (frequencies, allocation, the launch, its synchronise), on a one-layer model; median of `--table-repeats` builds, a child
  process per seq_len.

Every child runs under its own time limit; a child that fails ends the run. Writes profiles/rope_scaling_bench.json (or --out)."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLAMA3 = "llama3,factor=8,low=1,high=4,orig=8192"
PROMPT = [1, 2436, 385, 3686, 388, 1048, 22796, 118]


def open_library():
    import ctypes as C
    from llama_cu_awq_amd import api
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    return api


def child_tokens(args):
    from llama_cu_awq_amd import synth
    api = open_library()
    path = os.path.join(args.model_dir, "llama2_q4_synth_%s_seed20240229.bin" % args.model)
    if not os.path.exists(path):
        synth.write_model(path, args.model)
    t = api.Transformer(path, rope_scaling=None if args.scaling == "none" else args.scaling)
    t.generate_ids(PROMPT, args.ntok)
    runs = sorted(t.generate_ids(PROMPT, args.ntok)[1] for _ in range(4))
    print(json.dumps({"best": runs[-1], "median": 0.5 * (runs[1] + runs[2]), "rope_scaling": t.rope_scaling}))
    t.close()
    return 0


def child_table(args):
    from llama_cu_awq_amd import synth
    api = open_library()
    path = os.path.join(args.model_dir, "llama2_q4_synth_rope_table_%d.bin" % args.seq_len)
    synth.write_model(path, (256, 352, 1, 2, 2, 512, args.seq_len, 500000.0))          # one layer, head size 128
    for scaling in (None, LLAMA3):
        for _ in range(args.table_repeats + 1):
            api.Transformer(path, rope_scaling=scaling).close()
    os.remove(path)
    return 0


def run_child(argv, env, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child %r failed with status %d" % (argv, r.returncode))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libllama2_q4.so built from the parent commit; without it the parent column is left out")
    ap.add_argument("--model", default="7b")
    ap.add_argument("--ntok", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--table-repeats", type=int, default=5)
    ap.add_argument("--model-dir", default=os.environ.get("Q4_MODEL_DIR", "/tmp"))
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take (the first one writes the model file)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rope_scaling_bench.json"))
    ap.add_argument("--child", choices=("tokens", "table"), default=None)
    ap.add_argument("--scaling", default="none")
    ap.add_argument("--seq-len", type=int, default=2048)
    args = ap.parse_args()
    if args.child == "tokens":
        return child_tokens(args)
    if args.child == "table":
        return child_table(args)

    env = {k: v for k, v in os.environ.items() if k not in ("Q4_LIB_OVERRIDE", "Q4_DEBUG_ROPE", "Q4_ROPE_SCALING")}
    common = ["--model", args.model, "--ntok", str(args.ntok), "--model-dir", args.model_dir]
    columns = [("this_build_unscaled", None, "none"), ("this_build_llama3", None, LLAMA3)]
    if args.parent_lib:
        columns.insert(0, ("parent", os.path.abspath(args.parent_lib), "none"))
    res = {"model": args.model, "ntok": args.ntok, "rounds": args.rounds, "llama3_setting": LLAMA3, "tokens_per_s": {c[0]: [] for c in columns},
           "note": "tokens_per_s: per process the median of four timed greedy generations behind one warm one; processes interleaved parent, unscaled, "
                   "llama3, ...; spread = max - min of a column's medians. table_build_ms: q4_build_transformer's own report under Q4_DEBUG_ROPE=1"}
    for _ in range(args.rounds):
        for name, lib, scaling in columns:
            e = dict(env, Q4_LIB_OVERRIDE=lib) if lib else env
            out = run_child(["--child", "tokens", "--scaling", scaling] + common, e, args.limit).stdout
            row = json.loads(out.strip().splitlines()[-1])
            assert (row["rope_scaling"] is None) == (scaling == "none"), row
            res["tokens_per_s"][name].append(round(row["median"], 1))
            print(name, row, flush=True)
    summary = {}
    for name, meds in res["tokens_per_s"].items():
        s = sorted(meds)
        summary[name] = {"median_of_medians": s[len(s) // 2], "spread": round(s[-1] - s[0], 1)}
    res["summary"] = summary
    if "parent" in summary:
        base = summary["parent"]
        for name in ("this_build_unscaled", "this_build_llama3"):
            d = round(summary[name]["median_of_medians"] - base["median_of_medians"], 1)
            summary[name]["minus_parent"] = d
            summary[name]["within_parent_spread"] = abs(d) <= base["spread"]

    res["table_build_ms"] = {}
    for seq_len in (2048, 131072):
        err = run_child(["--child", "table", "--seq-len", str(seq_len), "--table-repeats", str(args.table_repeats), "--model-dir", args.model_dir],
                        dict(env, Q4_DEBUG_ROPE="1"), args.limit).stderr
        found = re.findall(r"rope table: (\d+) entries, scaling kind (\d), built in ([0-9.]+) ms", err)
        row = {"entries": int(found[0][0]), "table_bytes": 8 * int(found[0][0])}
        for kind, key in (("0", "unscaled"), ("2", "llama3")):
            ms = sorted([float(f[2]) for f in found if f[1] == kind][1:])          # (the first build of a kind is the warm one)
            row[key] = {"median": ms[len(ms) // 2], "best": ms[0], "worst": ms[-1], "builds": len(ms)}
        res["table_build_ms"][str(seq_len)] = row
        print("table", seq_len, row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
