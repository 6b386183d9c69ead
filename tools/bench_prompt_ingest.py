#!/usr/bin/env python3
"""Prompt ingest (csrc/prompt_pass.h, q4_set_prompt_ingest) measured on the flagship geometry: the time from q4_reset_sequence to the first generated
token for prompts of 8, 64, 128 and 250 tokens with the passes off (the per-token steps: what the library did before it had passes) and on, and the
time of one pass against the number of positions it takes. Writes profiles/prompt_ingest_bench.json (or the path given).
    tools/bench_prompt_ingest.py [out.json] [model] [repeats]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

from llama_cu_awq_amd import api, synth  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prompt_ingest_bench.json")
    model = sys.argv[2] if len(sys.argv) > 2 else "7b"
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    L = api.lib()
    api.check(L.q4_set_device(0))
    s = C.c_void_p()
    api.check(L.q4_stream_create(C.byref(s)))
    L.q4_set_stream(s)
    path = os.path.join(os.environ.get("Q4_MODEL_DIR", "/tmp"), "llama2_q4_synth_%s_seed20240229.bin" % model)
    if not os.path.exists(path):
        synth.write_model(path, model)
    t = api.Transformer(path)
    T = L.q4_get_prompt_ingest()
    rng = np.random.default_rng(7)

    def first_token_ms(prompt, ingest):
        """median milliseconds from the reset to the end of the prompt's last step: every prompt position and the first generated token"""
        L.q4_set_prompt_ingest(ingest)
        steps = len(prompt) + 1      # the loop's clock stops once the step BEHIND the one it queued last has ended: queue one more
        t.generate_ids(prompt, steps)                       # warm: graphs captured, scratch allocated
        return 1e3 * statistics.median(t.generate_ids(prompt, steps)[3] for _ in range(reps))

    res = {"model": model, "tokens_per_pass": T, "repeats": reps, "first_token": [], "pass_ms_by_positions": {}}
    for n in (8, 64, 128, 250):
        prompt = [1] + [int(x) for x in rng.integers(3, t.config.vocab_size, size=n - 1)]
        off, on = first_token_ms(prompt, 0), first_token_ms(prompt, T)
        res["first_token"].append({"prompt_tokens": n, "per_token_ms": round(off, 4), "passes_ms": round(on, 4), "ratio": round(off / on, 3)})
        print(res["first_token"][-1], flush=True)
    # one pass of n positions: a prompt of n + 1 tokens (n prompt-only positions, then the generating step) against the generating step alone
    base = first_token_ms([1], T)
    for n in range(2, T + 1):
        prompt = [1] + [int(x) for x in rng.integers(3, t.config.vocab_size, size=n)]
        before = L.q4_prompt_passes()
        ms = first_token_ms(prompt, T)
        assert L.q4_prompt_passes() > before, "no pass ran: this model or setting is not admitted"
        steps_ms = first_token_ms(prompt, 0)
        res["pass_ms_by_positions"][str(n)] = {"pass_ms": round(ms - base, 4), "per_token_steps_ms": round(steps_ms - base, 4)}
        print(n, res["pass_ms_by_positions"][str(n)], flush=True)
    L.q4_set_prompt_ingest(T)
    t.close()
    json.dump(res, open(out, "w"), indent=1, sort_keys=True)
    print("wrote", out)


if __name__ == "__main__":
    main()
