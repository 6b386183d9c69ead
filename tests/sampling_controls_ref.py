"""numpy float32 restatement of the sampling controls' launch (csrc/q4_logit_process.hip, include/llama2_q4.h): logit bias, repetition / presence /
frequency penalties over a window of the token ring, clamp and round, top-k on the monotone half key, min-p. Bit for bit what the kernel writes."""
import numpy as np

F = np.float32
NEUTRAL = dict(top_k=0, min_p=0.0, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_last_n=64)


def half_key(x):
    """the monotone 16-bit key of q4_logprobs.hip: larger value <=> larger key; -0 counts as +0; a NaN gets key 0, below -inf"""
    h = np.ascontiguousarray(x, dtype=np.float16).view(np.uint16).astype(np.int64)
    h = np.where(h == 0x8000, 0, h)
    nan = (h & 0x7FFF) > 0x7C00
    key = np.where(h & 0x8000, ~h & 0xFFFF, h | 0x8000)
    return np.where(nan, 0, key)


def window(tokens, pos, last_n):
    """ring entries tokens[max(0, pos + 1 - last_n) .. pos]"""
    if tokens is None or pos is None or last_n <= 0 or pos < 0:
        return np.zeros(0, dtype=np.int64)
    return np.asarray(tokens[max(0, pos + 1 - last_n): pos + 1], dtype=np.int64)


def _finish(v):
    """step 3: a finite value clamped to +-65504 and rounded to half (nearest even); an infinity stays; a NaN is the quiet NaN 0x7E00"""
    v = F(v)
    if np.isnan(v):
        return np.array([0x7E00], dtype=np.uint16).view(np.float16)[0]
    if np.isfinite(v):
        v = min(max(v, F(-65504.0)), F(65504.0))
    return np.float16(v)


def threshold(min_p):
    return F(np.log(F(min_p)))


def process(logits, top_k=0, min_p=0.0, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_last_n=64, logit_bias=None,
            tokens=None, pos=None):
    """the processed fp16 logits (a new array)"""
    x = np.array(logits, dtype=np.float16)
    n = x.shape[0]
    bias = dict(logit_bias or {})
    r, presence, frequency = F(repeat_penalty), F(presence_penalty), F(frequency_penalty)
    penalised = not (r == F(1.0) and presence == F(0.0) and frequency == F(0.0))
    win = window(tokens, pos, penalty_last_n) if penalised else np.zeros(0, dtype=np.int64)
    win = win[(win >= 0) & (win < n)]
    ids, counts = np.unique(win, return_counts=True)
    count = dict(zip(ids.tolist(), counts.tolist()))
    with np.errstate(all="ignore"):
        for i in sorted(set(bias) | set(count)):
            if not 0 <= i < n:
                continue
            v = F(x[i])
            if i in bias:
                v = F(v + F(bias[i]))
            c = count.get(i, 0)
            if c > 0:
                v = F(v / r) if v > 0 else F(v * r)
                pen = F(F(c) * frequency)
                v = F(v - F(pen + presence))
            x[i] = _finish(v)
        if top_k > 0 and top_k < n:
            order = np.lexsort((np.arange(n), -half_key(x)))
            x[order[top_k:]] = -np.inf
        if min_p > 0:
            m = F(x[int(np.lexsort((np.arange(n), -half_key(x)))[0])])      # the largest in the key order (a NaN only if every entry is one)
            keep = (x.astype(F) - m) >= threshold(min_p)      # (a NaN difference compares false: the entry goes)
            x[~keep] = -np.inf
    return x


def min_p_margin(logits, min_p, **kw):
    """the smallest |(l_i - m) - ln(min_p)| over the entries, relative to |ln(min_p)|, in float64 -- of the logits processed WITHOUT min-p (the test's
    condition on its inputs: nothing may lie within 2^-20 of the threshold)"""
    x = process(logits, min_p=0.0, **kw).astype(np.float64)
    t = np.log(np.float64(F(min_p)))
    fin = np.isfinite(x)
    if not fin.any():
        return np.inf
    d = np.abs((x[fin] - x[fin].max()) - t)
    return float(d.min() / abs(t))
