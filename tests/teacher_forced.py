"""What the step-level tests of the logit stages share: the raw logits of a finished run, teacher-forced through a model with nothing switched on, and
the tokens a run must have chosen according to the numpy reference of the sampling controls and the restated sampler."""
import ctypes as C

import numpy as np

import sampling_controls_ref as ref


def raw_logits(q4, path, tokens):
    """the sequence teacher-forced through a model WITHOUT controls, one graph replay per step: the raw fp16 logits of every position"""
    t = q4.Transformer(path)
    t.reset(tokens)
    out = []
    for pos in range(len(tokens) - 1):
        t.run_transformer_at(pos, 0)
        out.append(t.logits())
    t.close()
    return np.stack(out)


def predict(q4, orc, raw, tokens, n_prompt, controls, bias, mode, seed, sampled, first_coin=0):
    """what every generating step must have chosen: the reference over the raw logits and the ring window, then the argmax (lowest index) or the
    restated sampler at sampled = (temperature, topp) with the seed's coin stream (one coin per step, prompt steps included)"""
    L = q4.lib()
    state = C.c_ulonglong(seed)
    for _ in range(first_coin):
        L.random_f32(C.byref(state))
    out = np.array(tokens, dtype=np.int32).copy()
    for p in range(len(tokens) - 1):
        coin = L.random_f32(C.byref(state))
        if p < n_prompt - 1:
            continue
        x = ref.process(raw[p], tokens=tokens, pos=p, logit_bias=bias, **controls)
        if mode == "greedy":
            out[p + 1] = int(np.argmax(x.astype(np.float32)))
        else:
            out[p + 1] = orc.lib().orc_sample_topp(orc.f16_bits(x.copy()), x.shape[0], sampled[0], sampled[1], coin)
    return out
